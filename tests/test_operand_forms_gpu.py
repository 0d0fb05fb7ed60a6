"""Every native op of the convolution, resampling and fully connected families on operands that are NOT fresh dense tensors: views at an odd storage offset,
batch / channel slices, crops, steps, swapped axes, ``expand``ed and empty batches, 1 x 1 images cut out of larger ones (operand_forms.make).  The op's own
test file varies shapes on fresh ``torch.randn`` tensors; here the shape is the smallest that reaches each kernel family and the operand's FORM varies — one
operand at a time, plus one case with all of them awkward.  For each (op, operand, form):

  a. nothing raises; shape, dtype and strides of the result are those of the dense call;
  b. the result matches the fp64 CPU reference on the same values, within the bound of the op's own test file (imported, not copied);
  c. where the counters show the dense call's route, the result is bit-identical to the dense call's;
  d. the counters agree with the route table below;
  e. every input — the whole buffer it is a view of — is bit-identical afterwards, and no result shares storage with an input;
  f. gradient ops: ``torch.autograd.grad`` with an awkward ``gy`` matches the fp64 gradients within the same bounds, in the input's logical shape;
  g. an empty batch gives empty results of the right shape, launches nothing, and its weight gradient is zero.
  h. NaN-filled blocks of the result's size go back to the caching allocator first: an element no kernel stores shows as NaN (an aid, not an assertion).

ROUTES, per op, and what the C entry behind each operand does with a pointer that is off a 16-byte boundary or a tensor that is not dense (read from csrc/):

  conv2d_gradfix (p3d_conv2d_forward, p3d_conv2d_bwd_weight; fc shortcut: p3d_fc_forward)        x, w, gy: 'copy+native' for every form
      conv2d_forward -> plan_conv REFUSES x / relaid w off a boundary (conv2d.hip: "conv2d_nhwc: x, w and zeros128 must be 16-byte aligned"); the skinny 1x1
      kernels take x's vector path only when aligned (conv2d_grad.hip launch_skinny_1x1) but read ``weight`` and write ``y`` NEITHER checked NOR on a scalar path;
      the weight-gradient plan notes both images' alignment (note_operands) and has scalar loads for them; fc_forward REFUSES.  None takes strides: the host makes
      everything dense.  So: the host helper (modconv.kernel_operand) realigns every operand first, and only the guarded behaviour is run here.
  conv_layer (_ConvBiasAct -> p3d_conv2d_nhwc_ws; _Fc -> p3d_fc_forward)                        x, gy: 'copy+native'
      both entries REFUSE; same helper.
  Conv2dLayer / SynthesisLayer / ToRGBLayer / FullyConnectedLayer under no_grad (modconv)         alignment-only forms: 'copy+native'
      p3d_conv2d_nhwc*, p3d_up2_fir_*, p3d_fir4_bias_act_nhwc, p3d_fc_forward, p3d_conv3x3_torgb_f16 REFUSE; p3d_torgb_nhwc_f16 and p3d_modulate_weights check
      NOTHING (guarded by the helper).  A strided x is made channels-last by the layer itself before its predicate is asked (modconv.dense_input): 'copy+native'
      too — the generic route would answer an fp16 ToRGB in fp16 NHWC where the native one answers in fp32 NCHW.  Styles in any form: the affine's fc kernel reads rows at a stride of whole float4s in place
      ('native'), copies anything else ('copy+native').
  upfirdn2d (p3d_upfirdn2d)                                                                      every form 'native'
      takes element strides for x, f and y; the tiled / channels-last fast paths are chosen only for aligned pointers (upfirdn2d.hip: fast_path_ok), else the
      generic per-output kernel: a SCALAR path.
  bias_act (p3d_bias_act)                                                                        dense forms 'native', strided 'copy+native'
      ``aligned`` is a kernel argument (bias_act.hip: al16 of x, y, xref, yref, dy): a SCALAR path; the wrapper makes strided operands dense.

Forms the APIs cannot express, left out of the parameter lists: 'empty' and 'unit' for weights and filters (they would change the op, not the operand) and for
``gy`` alone (its shape is the result's: it follows x); 'empty' for the modulated layers (the reference's grouped convolution has no N = 0 either); 'batch_slice'
where an image is a multiple of 16 bytes says nothing new beyond 'dense' and is run on the 3-channel 5 x 5 shapes only; 'crop' / 'chan_slice' / 'hw_swapped' for
2-D operands.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import operand_forms as of
from conftest import rel_err
from oracle import ops_oracle as O
from test_conv_grad_gpu import GEOM as GRAD_GEOM, TOL as GRAD_TOL, _ref_op, _dev_op
from test_conv_layer_gpu import CASES as LAYER_CASES, FC_CASES
from test_ops_gpu import TOL as BIAS_ACT_TOL

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'f16': torch.float16}
LAYER_TOL = {torch.float32: 1e-5, torch.float16: 2e-3}       # test_conv_gpu.py: exact / bf16x3 fp32 1e-5, fp16 2e-3 (literals there)
UPFIRDN_TOL = {torch.float32: 2e-6, torch.float16: 2e-3}     # test_ops_gpu.test_upfirdn2d_cases (literals there)
VALUE_FORMS = ('expand', 'empty', 'unit')                    # forms whose values / shape differ from the dense tensor's: the reference follows them
COPIES = [0]


def _mods():
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.torch_utils.ops import conv2d_gradfix, modconv, conv_layer, upfirdn2d, bias_act
    return _lib, conv2d_gradfix, modconv, conv_layer, upfirdn2d, bias_act


@pytest.fixture()
def native(hip_lib):
    """conv2d_gradfix on (as in a training run), the copies of modconv.kernel_operand counted."""
    _lib, gradfix, modconv, *_ = _mods()
    prev, real = gradfix.enabled, modconv._fresh

    def counted(t, *a, **kw):
        COPIES[0] += 1
        return real(t, *a, **kw)
    gradfix.enabled, modconv._fresh = True, counted
    yield
    gradfix.enabled, modconv._fresh = prev, real


def counters():
    _lib, gradfix, modconv, *_ = _mods()
    c = {f: _lib.launch_count(f) for f in _lib.FAMILY}
    c.update({'gradfix_' + k: v for k, v in gradfix.native_calls.items()})
    c.update(fused_torgb=modconv.fused_torgb_calls, copies=COPIES[0])
    return c


def delta(c0):
    c1 = counters()
    return {k: c1[k] - c0[k] for k in c1}


def launches(d):
    from pix2pix3d_amd import _lib
    return sum(d[f] for f in _lib.FAMILY)


def kernels_of(d):
    """The route as the counters show it: everything but the count of operand copies."""
    return {k: v for k, v in d.items() if k != 'copies'}


def poison(*tensors):
    """(h) NaN-filled blocks back to the caching allocator: of these tensors' sizes (the results, where a dense call has shown them; the operands, which the
    results resemble, otherwise) and of every power of four from 1 KB to 16 MB (the workspaces: split-K partial tiles, weight re-layouts)."""
    sizes = [max(t.numel(), 1) * t.element_size() for t in tensors if t is not None] + [1 << k for k in range(10, 25, 2)]
    blocks = [torch.empty(nb + nb % 2, dtype=torch.uint8, device='cuda').view(torch.float16).fill_(float('nan')) for nb in sizes]
    del blocks


def vforms(forms):
    return tuple(sorted((k, f) for k, f in forms.items() if f in VALUE_FORMS))


def check_outputs(out, dense_out, ref, tol, same_route, what):
    errs = {}
    for k, want in ref.items():
        got = out[k]
        assert tuple(got.shape) == tuple(want.shape), (what, k, got.shape, want.shape)
        assert got.dtype == dense_out[k].dtype and got.stride() == dense_out[k].stride(), (what, k, got.stride(), dense_out[k].stride())      # (a)
        if want.numel() == 0:
            continue
        assert torch.isfinite(got).all(), (what, k, 'non-finite: an element no kernel stored?')
        errs[k] = rel_err(got.detach().double().cpu(), want)
    print(what, errs)
    assert all(e < tol for e in errs.values()), (what, errs, tol)                                 # (b), (f)
    if same_route:
        for k in ref:
            assert torch.equal(out[k], dense_out[k]), (what, k, 'differs from the dense call on the same route')      # (c)


def run_guarded(call, operands, results_like):
    """Run ``call(operands)`` with (e) every input's whole buffer compared before and after, (h) poison, and the counters' delta."""
    bases = {k: of.base_of(t) for k, t in operands.items() if t.numel()}
    before = {k: b.clone() for k, b in bases.items()}
    poison(*(results_like or operands.values()))
    c0 = counters()
    out = call(operands)
    torch.cuda.synchronize()
    d = delta(c0)
    for k, b in bases.items():
        assert torch.equal(b, before[k]), (k, 'an input buffer was written')
    for k, o in out.items():
        for name, t in operands.items():
            assert not of.shares_storage(o, t), (k, name, 'the result shares storage with an input')
    return out, d


def run_warm(call, operands):
    """The dense call of a LAYER, on its second run: the first builds the derived forms of the weights that are kept per weight version (a launch and a copy of its own)."""
    run_guarded(call, operands, ())
    return run_guarded(call, operands, ())


def expect_route(route, d, dense_d, what, copies=None):
    """(d) the counters against the route table.  'native': the dense call's kernels and no more copies than it made; 'copy+native': the same kernels;
    'fallback': other launches than the dense call's (torch's operators, or the unfused formulation on the library's own kernels); 'none': no launch of any family."""
    assert d['gradfix_aten'] == dense_d['gradfix_aten'] or route == 'fallback', (what, d)
    if route == 'native':
        assert kernels_of(d) == kernels_of(dense_d) and d['copies'] == dense_d['copies'], (what, d, dense_d)
    elif route == 'copy+native':                                 # copies: 'more' where the helper is known to copy this form, 'same' where the operand is read in place
        assert kernels_of(d) == kernels_of(dense_d) and d['copies'] >= dense_d['copies'], (what, d, dense_d)
        assert copies != 'more' or d['copies'] > dense_d['copies'], (what, 'no copy was made', d, dense_d)
        assert copies != 'same' or d['copies'] == dense_d['copies'], (what, 'a copy was made', d, dense_d)
    elif route == 'fallback':
        assert kernels_of(d) != kernels_of(dense_d), (what, d, dense_d)
    else:
        assert route == 'none' and all(v == 0 for k, v in d.items() if k != 'copies'), (what, d)


# ---- conv2d_gradfix: forward, data gradient, weight gradient ------------------------------------------------------------------------------------------------------

GEOMS = {g[0]: g for g in GRAD_GEOM}
GEOMS['fc1x1'] = ('fc1x1', False, 1, 1, 512, 512, 1, 1, 4, 0)           # a 1x1 convolution of 1x1 images: the fully connected shortcut (fp32)
GEOMS['rgb5x5'] = ('rgb5x5', False, 3, 1, 3, 64, 5, 5, 2, 0)            # an image of 3 x 5 x 5 elements: no multiple of 16 bytes in either dtype (channel padding route)
GEOMS['rgb5x5_1x1'] = ('rgb5x5_1x1', False, 1, 1, 3, 64, 5, 5, 2, 0)    # ... on the skinny 1x1 kernel
FULL_GEOM = 'same3x3'
OTHER_GEOMS = ['same1x1', 'down3x3_odd', 'up3x3', 'up3x3_big', 'fromrgb', 'torgb', 'fold4x4', 'fc1x1']
X_FORMS = [f for f in of.FORMS]
W_FORMS = ['offset1', 'offset8', 'chan_slice', 'crop', 'step', 'hw_swapped', 'expand']
GY_FORMS = ['offset1', 'offset8', 'batch_slice', 'chan_slice', 'crop', 'step', 'hw_swapped', 'expand']


def _gradfix_params():
    p = []
    for dt in DTYPES:
        for layout in ('nhwc', 'nchw'):
            p += [(FULL_GEOM, dt, layout, 'x', f) for f in X_FORMS]
        p += [(FULL_GEOM, dt, 'nhwc', 'w', f) for f in W_FORMS] + [(FULL_GEOM, dt, 'nhwc', 'gy', f) for f in GY_FORMS]
        p += [(FULL_GEOM, dt, 'nhwc', 'all', 'mixed'), (FULL_GEOM, dt, 'nchw', 'all', 'mixed')]
        for name in OTHER_GEOMS:
            if name == 'fc1x1' and dt == 'f16':
                continue                                         # (the shortcut is fp32 only; fp16 1x1 images take the kernel of 'same1x1')
            p += [(name, dt, 'nhwc', 'x', 'dense')] + [(name, dt, 'nhwc', k, 'offset1') for k in ('x', 'w', 'gy')] + [(name, dt, 'nhwc', 'all', 'mixed')]
        for name in ('rgb5x5', 'rgb5x5_1x1'):
            p += [(name, dt, layout, 'x', f) for layout in ('nhwc', 'nchw') for f in ('dense', 'batch_slice')] + [(name, dt, 'nhwc', 'gy', 'offset8'), (name, dt, 'nhwc', 'all', 'mixed')]
    return p


MIXED = {'x': 'offset1', 'w': 'offset8', 'gy': 'crop'}


@functools.lru_cache(maxsize=None)
def _gradfix_values(name, dt, vf):
    """Dense CPU operands (in the device dtype) and the fp64 reference of y, gx, gw on their values; once per (geometry, dtype, value-changing forms)."""
    geom, dtype, vf = GEOMS[name], DTYPES[dt], dict(vf)
    _, tr, k, stride, ci, co, h, w, n, op = geom
    g = torch.Generator().manual_seed(len(name) + 17)
    x = torch.randn(n, ci, h, w, generator=g).to(dtype)
    wt = (torch.randn(*((ci, co) if tr else (co, ci)), k, k, generator=g) / np.sqrt(ci * k * k)).to(dtype)
    x, wt = of.values(vf.get('x', 'dense'), x), of.values(vf.get('w', 'dense'), wt)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    yr = _ref_op(xr, wr, geom)
    gy = of.values(vf.get('gy', 'dense'), torch.randn(yr.shape, generator=g).to(dtype))
    if yr.numel():
        gxr, gwr = torch.autograd.grad(yr, [xr, wr], gy.double())
    else:
        gxr, gwr = torch.zeros_like(xr), torch.zeros_like(wr)
    return dict(x=x, w=wt, gy=gy), dict(y=yr.detach(), gx=gxr, gw=gwr)


def _gradfix_call(geom):
    def call(ops):
        x, w = ops['x'].requires_grad_(True), ops['w'].requires_grad_(True)
        y = _dev_op(x, w, geom)
        gx, gw = torch.autograd.grad(y, [x, w], ops['gy'])
        return dict(y=y.detach(), gx=gx, gw=gw)
    return call


def _device_operands(dense, forms, layouts):
    return {k: of.make(forms.get(k, 'dense'), t.cuda(), layouts.get(k, 'nchw')) for k, t in dense.items()}


@functools.lru_cache(maxsize=None)
def _gradfix_dense(name, dt, layout, vf):
    dense, ref = _gradfix_values(name, dt, vf)
    ops = _device_operands(dense, {}, dict(x=layout, gy=layout))
    return run_guarded(_gradfix_call(GEOMS[name]), ops, ())


@pytest.mark.parametrize('name,dt,layout,operand,form', _gradfix_params(), ids=lambda v: str(v))
def test_conv2d_gradfix(native, name, dt, layout, operand, form):
    forms = dict(MIXED) if operand == 'all' else {operand: form}
    if forms.get('x') in ('empty', 'unit'):
        forms['gy'] = 'dense'                                    # gy has the result's shape: it follows x
    vf = vforms(forms)
    dense, ref = _gradfix_values(name, dt, vf)
    dense_out, dense_d = _gradfix_dense(name, dt, layout, vf)
    what = ('conv2d_gradfix', name, dt, layout, operand, form)
    assert dense_d['gradfix_aten'] == 0 and (form == 'empty' or (dense_d['gradfix_forward'], dense_d['gradfix_weight_grad']) == (2, 1)), (what, dense_d)
    ops = _device_operands(dense, forms, dict(x=layout, gy=layout))
    out, d = run_guarded(_gradfix_call(GEOMS[name]), ops, (dense_out['y'], dense_out['gx'], dense_out['gw']))
    route = 'none' if form == 'empty' else ('native' if forms == {operand: 'dense'} else 'copy+native')
    # channels-last operands are handed on as they are when they can be: every other form costs a copy of the helper's (an NCHW operand is copied either way);
    # a batch slice of whole 16-byte images is as good as dense
    aligned_slice = form == 'batch_slice' and not name.startswith('rgb5x5')
    expect_route(route, d, dense_d, what, copies='same' if aligned_slice else ('more' if layout == 'nhwc' else None))
    assert d['gradfix_aten'] == 0, (what, d)
    check_outputs(out, dense_out, ref, GRAD_TOL[DTYPES[dt]], kernels_of(d) == kernels_of(dense_d), what)
    if form == 'empty':
        assert out['y'].shape[0] == 0 and out['gx'].shape[0] == 0 and not out['gw'].any()      # (g)


# ---- conv2d_resample: up, down and same, the filter as a view too ---------------------------------------------------------------------------------------------------

RESAMPLE = {'up': dict(up=2, down=1, k=3, ci=64, co=64, h=9, w=11), 'down': dict(up=1, down=2, k=3, ci=64, co=64, h=17, w=14), 'same': dict(up=1, down=1, k=3, ci=64, co=32, h=10, w=7)}


@functools.lru_cache(maxsize=None)
def _resample_values(name, dt, vf):
    from pix2pix3d_amd.torch_utils.ops import conv2d_resample, upfirdn2d
    c, dtype, vf = RESAMPLE[name], DTYPES[dt], dict(vf)
    g = torch.Generator().manual_seed(len(name) + 5)
    x = of.values(vf.get('x', 'dense'), torch.randn(2, c['ci'], c['h'], c['w'], generator=g).to(dtype))
    wt = (torch.randn(c['co'], c['ci'], c['k'], c['k'], generator=g) / np.sqrt(c['ci'] * 9)).to(dtype)
    f = upfirdn2d.setup_filter([1, 3, 3, 1])
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    yr = conv2d_resample.conv2d_resample(xr, wr, f=f, up=c['up'], down=c['down'], padding=1, flip_weight=c['up'] == 1)      # CPU: torch's own operators, fp64
    gy = torch.randn(yr.shape, generator=g).to(dtype)
    gxr, gwr = torch.autograd.grad(yr, [xr, wr], gy.double())
    return dict(x=x, w=wt, f=f, gy=gy), dict(y=yr.detach(), gx=gxr, gw=gwr)


def _resample_call(c):
    from pix2pix3d_amd.torch_utils.ops import conv2d_resample

    def call(ops):
        x, w = ops['x'].requires_grad_(True), ops['w'].requires_grad_(True)
        y = conv2d_resample.conv2d_resample(x, w, f=ops['f'], up=c['up'], down=c['down'], padding=1, flip_weight=c['up'] == 1)
        gx, gw = torch.autograd.grad(y, [x, w], ops['gy'])
        return dict(y=y.detach(), gx=gx, gw=gw)
    return call


@functools.lru_cache(maxsize=None)
def _resample_dense(name, dt, vf):
    dense, ref = _resample_values(name, dt, vf)
    return run_guarded(_resample_call(RESAMPLE[name]), _device_operands(dense, {}, dict(x='nhwc', gy='nhwc')), ())


@pytest.mark.parametrize('operand,form', [('x', 'dense'), ('x', 'offset1'), ('x', 'chan_slice'), ('x', 'expand'), ('w', 'offset8'), ('f', 'offset1'), ('f', 'step'), ('f', 'transposed'),
                                          ('gy', 'crop'), ('all', 'mixed')])
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('name', list(RESAMPLE))
def test_conv2d_resample(native, name, dt, operand, form):
    forms = dict(MIXED, f='step') if operand == 'all' else {operand: form}
    vf = vforms(forms)
    dense, ref = _resample_values(name, dt, vf)
    dense_out, dense_d = _resample_dense(name, dt, vf)
    what = ('conv2d_resample', name, dt, operand, form)
    ops = _device_operands({k: v for k, v in dense.items() if k != 'f'}, forms, dict(x='nhwc', gy='nhwc'))
    f = dense['f'].cuda()
    ops['f'] = of.make_2d('transposed', f) if forms.get('f') == 'transposed' else of.make(forms.get('f', 'dense'), f)
    out, d = run_guarded(_resample_call(RESAMPLE[name]), ops, tuple(dense_out.values()))
    # the filter goes to upfirdn2d, which reads it by strides: no copy; a weight off its boundary is copied by the helper
    expect_route('native' if forms == {operand: 'dense'} else 'copy+native', d, dense_d, what, copies='same' if operand == 'f' else ('more' if operand == 'w' and name != 'up' else None))      # (the up-sampling route mirrors the weight into a fresh tensor first)
    assert d['gradfix_aten'] == 0 and dense_d['gradfix_aten'] == 0 and dense_d['gradfix_forward'] == 2, (what, d, dense_d)
    check_outputs(out, dense_out, ref, GRAD_TOL[DTYPES[dt]], forms.get('f', 'dense') in ('dense', 'transposed'), what)


# ---- conv_layer: Conv2dLayer and FullyConnectedLayer in training passes, one launch each, with gradients -----------------------------------------------------------

def _fp64(layer):
    """A copy of the layer on the CPU in fp64 (its resampling filter stays the float32 tensor the ops ask for)."""
    ref = copy.deepcopy(layer).cpu().double()
    if getattr(ref, 'resample_filter', None) is not None:
        ref.resample_filter = ref.resample_filter.float()
    return ref


def _layer_ref(layer, x64, gy64, **kw):
    """The layer's own formulation on the CPU in fp64 (torch's operators): y and the gradients of <y, gy>."""
    ref = _fp64(layer)
    xr = x64.clone().requires_grad_(True)
    y = ref(xr, **kw)
    gy = gy64(y)
    if y.numel() == 0:
        return dict(y=y.detach()), gy
    grads = torch.autograd.grad(y, [xr] + list(ref.parameters()), gy.double(), allow_unused=True)
    out = dict(y=y.detach(), gx=grads[0])
    out.update({'g_' + k: v for (k, _), v in zip(ref.named_parameters(), grads[1:]) if v is not None})
    return out, gy


@functools.lru_cache(maxsize=None)
def _conv_layer_setup(idx, dt, vf):
    from pix2pix3d_amd.training.networks_stylegan2 import Conv2dLayer
    name, ci, co, k, down, act, bias, clamp, gain, h, n = LAYER_CASES[idx]
    dtype, vf = DTYPES[dt], dict(vf)
    torch.manual_seed(7 + idx)
    layer = Conv2dLayer(ci, co, k, bias=bias, activation=act, down=down, conv_clamp=clamp)
    if bias:
        with torch.no_grad():
            layer.bias.copy_(torch.randn(co) * 0.3)
    g = torch.Generator().manual_seed(idx)
    x = of.values(vf.get('x', 'dense'), torch.randn(n, ci, h, h, generator=g).to(dtype))
    ref, gy = _layer_ref(layer, x.double(), lambda y: of.values(vf.get('gy', 'dense'), torch.randn(y.shape, generator=g).to(dtype)), gain=gain)
    return layer.cuda(), gain, dict(x=x, gy=gy), ref


def _module_call(layer, **kw):
    def call(ops):
        for p in layer.parameters():
            p.grad = None
        x = ops['x'].requires_grad_(True)
        y = layer(x, **kw)
        if y.numel() == 0:
            return dict(y=y.detach())
        names = [k for k, _ in layer.named_parameters()]
        grads = torch.autograd.grad(y, [x] + list(layer.parameters()), ops['gy'], allow_unused=True)
        out = dict(y=y.detach(), gx=grads[0])
        out.update({'g_' + k: v for k, v in zip(names, grads[1:]) if v is not None})
        return out
    return call


@functools.lru_cache(maxsize=None)
def _conv_layer_dense(idx, dt, vf):
    layer, gain, dense, ref = _conv_layer_setup(idx, dt, vf)
    return run_warm(_module_call(layer, gain=gain), _device_operands(dense, {}, dict(x='nhwc', gy='nhwc')))


CONV_LAYER_FORMS = [('x', f) for f in ('dense',) + of.ALIGNMENT_FORMS[:2] + of.STRIDED_FORMS + ('empty',)] + [('gy', f) for f in ('offset1', 'offset8', 'crop', 'expand')] + [('all', 'mixed')]


@pytest.mark.parametrize('operand,form', CONV_LAYER_FORMS)
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('idx', [0, 1], ids=[LAYER_CASES[0][0], LAYER_CASES[1][0]])
def test_conv_layer(native, idx, dt, operand, form):
    _lib, gradfix, modconv, conv_layer, *_ = _mods()
    forms = dict(x='offset1', gy='crop') if operand == 'all' else {operand: form}
    vf = vforms(forms)
    layer, gain, dense, ref = _conv_layer_setup(idx, dt, vf)
    c0 = dict(conv_layer.calls)
    dense_out, dense_d = _conv_layer_dense(idx, dt, vf)
    what = ('conv_layer', LAYER_CASES[idx][0], dt, operand, form)
    out, d = run_guarded(_module_call(layer, gain=gain), _device_operands(dense, forms, dict(x='nhwc', gy='nhwc')), tuple(dense_out.values()))
    if form == 'empty':
        assert d['conv'] == 0 and d['gradfix_aten'] == 0 and out['y'].shape[0] == 0 and out['y'].shape[1:] == dense_out['y'].shape[1:], (what, d)
        return
    assert conv_layer.calls['forward'] > c0['forward'], (what, 'the one-launch layer did not run')
    # x reaches the convolution as it is only in the layer without down-sampling (the other one filters it first: upfirdn2d reads strides, its result is fresh);
    # gy goes through bias_act's gradient operator (a scalar path, a dense copy of torch's for strided forms), whose result is fresh
    expect_route('native' if forms == {operand: 'dense'} else 'copy+native', d, dense_d, what, copies='more' if idx == 0 and 'x' in forms else 'same')
    same = kernels_of(d) == kernels_of(dense_d)
    if dt == 'f32':                                              # test_conv_layer_gpu: fp32 2e-5 = GRAD_TOL, here against fp64
        return check_outputs(out, dense_out, ref, GRAD_TOL[torch.float32], same, what)
    # fp16, as test_conv_layer_gpu holds it (its literals): the output to 2e-3 — here against fp64 —; the gradients against the UNFUSED formulation on the same
    # kernels, any entry to 0.2 of the largest and 3 % in L2: the device rounds weight * gain to fp16, a few pre-activations per ten thousand land on the other
    # side of the leaky ReLU's kink, and a gradient entry fed by one moves by a few per cent of the largest (dense call against fp64: gx 3.9e-2, g_weight 2.7e-2)
    check_outputs(out, dense_out, dict(y=ref['y']), 2e-3, same, what)
    unfused = _conv_layer_unfused(idx, dt, vf)
    assert set(out) == set(unfused) == set(dense_out)
    for k in out:
        a, b = out[k].double().cpu(), unfused[k]
        assert a.shape == b.shape == ref[k].shape
        e, l2 = rel_err(a, b), float((a - b).norm() / b.norm().clamp_min(1e-12))
        assert e < 0.2 and l2 < 3e-2, (what, k, e, l2)
        assert not same or torch.equal(out[k], dense_out[k]), (what, k)


@functools.lru_cache(maxsize=None)
def _conv_layer_unfused(idx, dt, vf):
    conv_layer = _mods()[3]
    layer, gain, dense, ref = _conv_layer_setup(idx, dt, vf)
    prev, conv_layer.enabled = conv_layer.enabled, False
    try:
        out = _module_call(layer, gain=gain)(_device_operands(dense, {}, dict(x='nhwc', gy='nhwc')))
    finally:
        conv_layer.enabled = prev
    return {k: v.double().cpu() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _fc_layer_setup(vf):
    from pix2pix3d_amd.training.networks_stylegan2 import FullyConnectedLayer
    name, fin, fout, act, bias, lrm, n = FC_CASES[0]
    vf = dict(vf)
    torch.manual_seed(11)
    layer = FullyConnectedLayer(fin, fout, bias=bias, activation=act, lr_multiplier=lrm, bias_init=0.3)
    g = torch.Generator().manual_seed(5)
    x = of.values(vf.get('x', 'dense'), torch.randn(n, fin, generator=g))
    ref, gy = _layer_ref(layer, x.double(), lambda y: of.values(vf.get('gy', 'dense'), torch.randn(y.shape, generator=g)))
    return layer.cuda(), dict(x=x, gy=gy), ref


@functools.lru_cache(maxsize=None)
def _fc_layer_dense(vf):
    layer, dense, ref = _fc_layer_setup(vf)
    return run_warm(_module_call(layer), _device_operands(dense, {}, {}))


@pytest.mark.parametrize('operand,form', [('x', f) for f in ('dense', 'offset1', 'offset8', 'step', 'expand', 'unit')] + [('gy', f) for f in ('offset1', 'offset8', 'step', 'expand')] + [('all', 'mixed')])
def test_fully_connected_layer_in_training(native, operand, form):
    conv_layer = _mods()[3]
    forms = dict(x='offset1', gy='step') if operand == 'all' else {operand: form}
    if forms.get('x') == 'unit':
        forms['gy'] = 'dense'
    vf = vforms(forms)
    layer, dense, ref = _fc_layer_setup(vf)
    dense_out, dense_d = _fc_layer_dense(vf)
    c0 = dict(conv_layer.calls)
    what = ('fc_layer', operand, form)
    out, d = run_guarded(_module_call(layer), _device_operands(dense, forms, {}), tuple(dense_out.values()))
    assert conv_layer.calls['forward'] > c0['forward'] and conv_layer.calls['backward'] > c0['backward'], what
    expect_route('native' if forms == {operand: 'dense'} else 'copy+native', d, dense_d, what, copies='more' if form in ('offset1', 'offset8', 'mixed') else None)
    check_outputs(out, dense_out, ref, GRAD_TOL[torch.float32], kernels_of(d) == kernels_of(dense_d), what)


# ---- the inference layers on the modconv routes (no_grad) ----------------------------------------------------------------------------------------------------------------

def _synthesis(ci, co, res, up, dt):
    from pix2pix3d_amd.training.networks_stylegan2 import SynthesisLayer
    layer = SynthesisLayer(ci, co, w_dim=32, resolution=res * up, up=up, conv_clamp=256, channels_last=dt == 'f16').eval().requires_grad_(False)
    layer.noise_strength.fill_(0.2)
    layer.bias.normal_()
    return layer, dict(noise_mode='const', fused_modconv=True), (ci, res)


def _torgb(ci, co, res, dt):
    from pix2pix3d_amd.training.networks_stylegan2 import ToRGBLayer
    layer = ToRGBLayer(ci, co, w_dim=32, conv_clamp=256, channels_last=dt == 'f16').eval().requires_grad_(False)
    layer.bias.normal_()
    return layer, dict(fused_modconv=True), (ci, res)


MOD_LAYERS = {
    'syn_up1': lambda dt: _synthesis(128, 64, 32, 1, dt),
    'syn_up2': lambda dt: _synthesis(128, 64, 32, 2, dt),
    'syn_4x4': lambda dt: _synthesis(512, 512, 4, 1, dt),            # fp32: the shared-weight form, split-K
    'torgb_3': lambda dt: _torgb(128, 3, 32, dt),                     # fp16: the streaming kernel
    'torgb_wide': lambda dt: _torgb(64, 96, 32, dt),                  # a 1x1 through the matrix-core kernel
}
MOD_X_FORMS = ['dense', 'offset1', 'offset8', 'chan_slice', 'hw_swapped', 'expand']
MOD_W_FORMS = ['offset1', 'offset8', 'step', 'expand', 'ws_slice']
GENERIC_TOL = {torch.float32: 2e-5, torch.float16: 6e-3}       # test_conv_gpu.test_synthesis_layer_native_vs_generic (literals there)


@functools.lru_cache(maxsize=None)
def _mod_setup(name, dt, vf):
    vf = dict(vf)
    torch.manual_seed(len(name))
    layer, kw, (ci, res) = MOD_LAYERS[name](dt)
    g = torch.Generator().manual_seed(3)
    x = of.values(vf.get('x', 'dense'), torch.randn(2, ci, res, res, generator=g).to(DTYPES[dt]))
    w = of.values(vf.get('w', 'dense'), torch.randn(2, 32, generator=g))
    with torch.no_grad():
        ref = _fp64(layer)(x.double(), w.double(), **kw)       # CPU, fp64: the generic formulation on torch's operators
    return layer.cuda(), kw, dict(x=x, w=w), dict(y=ref)


def _mod_call(layer, kw):
    def call(ops):
        with torch.no_grad():
            return dict(y=layer(ops['x'], ops['w'], **kw))
    return call


@functools.lru_cache(maxsize=None)
def _mod_dense(name, dt, vf):
    layer, kw, dense, ref = _mod_setup(name, dt, vf)
    return run_warm(_mod_call(layer, kw), _device_operands(dense, {}, dict(x='nhwc')))


@pytest.mark.parametrize('operand,form', [('x', f) for f in MOD_X_FORMS] + [('w', f) for f in MOD_W_FORMS] + [('all', 'mixed')])
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('name', list(MOD_LAYERS))
def test_modulated_layers_in_inference(native, name, dt, operand, form):
    _lib, gradfix, modconv, *_ = _mods()
    forms = dict(x='offset1', w='ws_slice') if operand == 'all' else {operand: form}
    vf = vforms(forms)
    layer, kw, dense, ref = _mod_setup(name, dt, vf)
    dense_out, dense_d = _mod_dense(name, dt, vf)
    what = ('modconv', name, dt, operand, form)
    assert launches(dense_d) >= 1 and dense_d['gradfix_aten'] == 0, (what, dense_d, 'the dense call is off the native kernels')
    ops = _device_operands(dict(x=dense['x']), forms, dict(x='nhwc'))
    wd = dense['w'].cuda()
    ops['w'] = of.make_2d('ws_slice', wd) if forms.get('w') == 'ws_slice' else of.make(forms.get('w', 'dense'), wd)
    out, d = run_guarded(_mod_call(layer, kw), ops, tuple(dense_out.values()))
    if forms == {operand: 'dense'} or forms == {'w': 'ws_slice'}:
        route = 'native'
    else:
        route = 'copy+native'
    # a dense x or latent off its boundary, and a latent with a column stride, are copied by the helper; a strided x by the layer (torch's copy, not counted)
    known = form in ('offset1', 'offset8', 'mixed') or (operand, form) == ('w', 'step')
    expect_route(route, d, dense_d, what, copies='more' if known else None)
    same = kernels_of(d) == kernels_of(dense_d)
    check_outputs(out, dense_out, ref, LAYER_TOL[DTYPES[dt]], same, what)
    generic = _mod_generic(name, dt, vf)                         # ... and against the generic formulation on the device
    e = rel_err(out['y'].double().cpu(), generic)
    print(what, 'vs modconv.enabled = False', e)
    assert e < GENERIC_TOL[DTYPES[dt]], (what, e)


@functools.lru_cache(maxsize=None)
def _mod_generic(name, dt, vf):
    modconv = _mods()[2]
    layer, kw, dense, ref = _mod_setup(name, dt, vf)
    modconv.enabled = False
    try:
        with torch.no_grad():
            return layer(dense['x'].cuda().contiguous(memory_format=torch.channels_last), dense['w'].cuda(), **kw).double().cpu()
    finally:
        modconv.enabled = True


PLAIN = {'conv_down': dict(ci=64, co=128, k=3, down=2, res=64, act='lrelu'), 'conv_1x1': dict(ci=64, co=96, k=1, down=1, res=12, act='linear')}


@functools.lru_cache(maxsize=None)
def _plain_setup(name, dt, vf):
    from pix2pix3d_amd.training.networks_stylegan2 import Conv2dLayer
    c, vf = PLAIN[name], dict(vf)
    torch.manual_seed(9)
    layer = Conv2dLayer(c['ci'], c['co'], c['k'], activation=c['act'], down=c['down'], conv_clamp=256).eval().requires_grad_(False)
    layer.bias.normal_()
    x = of.values(vf.get('x', 'dense'), torch.randn(2, c['ci'], c['res'], c['res'], generator=torch.Generator().manual_seed(2)).to(DTYPES[dt]))
    with torch.no_grad():
        ref = _fp64(layer)(x.double())
    return layer.cuda(), dict(x=x), dict(y=ref)


@functools.lru_cache(maxsize=None)
def _plain_dense(name, dt, vf):
    layer, dense, ref = _plain_setup(name, dt, vf)
    return run_warm(lambda ops: dict(y=layer(ops['x'])), _device_operands(dense, {}, dict(x='nhwc')))


@pytest.mark.parametrize('form', ['dense', 'offset1', 'offset8', 'chan_slice', 'expand', 'empty'])
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('name', list(PLAIN))
def test_plain_conv_layer_in_inference(native, name, dt, form):
    vf = vforms({'x': form})
    layer, dense, ref = _plain_setup(name, dt, vf)
    with torch.no_grad():
        dense_out, dense_d = _plain_dense(name, dt, vf)
        out, d = run_guarded(lambda ops: dict(y=layer(ops['x'])), _device_operands(dense, {'x': form}, dict(x='nhwc')), tuple(dense_out.values()))
    what = ('plain_layer', name, dt, form)
    if form == 'empty':
        assert d['conv'] == 0 and out['y'].shape == ref['y'].shape and out['y'].shape[0] == 0, (what, d)
        return
    assert dense_d['conv'] >= 1 and dense_d['gradfix_forward'] == 0, (what, dense_d)
    # (the down-sampling layer filters x first — upfirdn2d reads strides — and convolves the fresh result; the 1x1 layer's x reaches the helper)
    expect_route('native' if form == 'dense' else 'copy+native', d, dense_d, what, copies='more' if name == 'conv_1x1' and form in ('offset1', 'offset8') else None)
    check_outputs(out, dense_out, ref, LAYER_TOL[DTYPES[dt]], kernels_of(d) == kernels_of(dense_d), what)


FC_INFER = {'affine96': (512, 96, 'linear'), 'camera': (25, 64, 'lrelu')}


@functools.lru_cache(maxsize=None)
def _fc_infer_setup(name, rows, vf):
    from pix2pix3d_amd.training.networks_stylegan2 import FullyConnectedLayer
    fin, fout, act = FC_INFER[name]
    torch.manual_seed(4)
    layer = FullyConnectedLayer(fin, fout, activation=act, bias_init=0.3).eval().requires_grad_(False)
    x = of.values(dict(vf).get('x', 'dense'), torch.randn(rows, fin, generator=torch.Generator().manual_seed(rows)))
    with torch.no_grad():
        ref = _fp64(layer)(x.double())
    return layer.cuda(), dict(x=x), dict(y=ref)


@functools.lru_cache(maxsize=None)
def _fc_infer_dense(name, rows, vf):
    layer, dense, ref = _fc_infer_setup(name, rows, vf)
    return run_warm(lambda ops: dict(y=layer(ops['x'])), _device_operands(dense, {}, {}))


@pytest.mark.parametrize('form', ['dense', 'offset1', 'offset8', 'batch_slice', 'step', 'expand', 'ws_slice'])
@pytest.mark.parametrize('rows', [1, 4])
@pytest.mark.parametrize('name', list(FC_INFER))
def test_fully_connected_layer_in_inference(native, name, rows, form):
    vf = vforms({'x': form})
    layer, dense, ref = _fc_infer_setup(name, rows, vf)
    with torch.no_grad():
        dense_out, dense_d = _fc_infer_dense(name, rows, vf)
        xd = dense['x'].cuda()
        ops = dict(x=of.make_2d('ws_slice', xd) if form == 'ws_slice' else of.make(form, xd))
        out, d = run_guarded(lambda ops: dict(y=layer(ops['x'])), ops, tuple(dense_out.values()))
    what = ('fc', name, rows, form)
    assert launches(dense_d) == 1, (what, dense_d)              # the one-launch fc kernel
    # rows at a stride of whole float4s from a boundary are read in place; 25 camera parameters are zero-padded into a fresh tensor whatever their form;
    # anything else of the 512-wide rows is copied by the helper
    if form in ('dense', 'ws_slice'):
        route, copies = ('native', None) if form == 'dense' else ('copy+native', 'same')
    else:
        route, copies = 'copy+native', ('more' if name == 'affine96' and form in ('offset1', 'offset8', 'step') else None)
    expect_route(route, d, dense_d, what, copies=copies)
    check_outputs(out, dense_out, ref, LAYER_TOL[torch.float32], kernels_of(d) == kernels_of(dense_d), what)


# ---- the wide-ToRGB fusion and the noise image: refused from Python, nothing launched -------------------------------------------------------------------------

def test_a_misshapen_noise_image_never_reaches_a_kernel(native):
    """synthesis_layer, up2_fir, fir4_bias_act, conv2d and conv3x3_torgb_wide hand ``noise`` to a kernel by pointer: another size raises before any launch."""
    _lib, gradfix, modconv, *_ = _mods()
    n, ci, co, h = 2, 64, 64, 16
    weight, styles, bias = torch.randn(co, ci, 3, 3, device='cuda'), torch.randn(n, ci, device='cuda'), torch.zeros(co, device='cuda')
    f = torch.ones(4, 4, device='cuda') / 16
    strength = torch.tensor(0.1, device='cuda')
    for dtype in (torch.float32, torch.float16):
        x = torch.randn(n, ci, h, h, device='cuda').to(dtype).contiguous(memory_format=torch.channels_last)
        wmod = torch.zeros(n, co, 9, ci, device='cuda', dtype=dtype)
        y_t = torch.zeros(n, co, 2 * h + 1, 2 * h + 1, device='cuda', dtype=dtype).contiguous(memory_format=torch.channels_last)
        for up in (1, 2):
            for bad in (torch.zeros(up * h, up * h // 2, device='cuda'), torch.zeros(h // 2, h // 2, device='cuda'), torch.zeros(1, 1, up * h, up * h, device='cuda')):
                c0 = counters()
                with torch.no_grad(), pytest.raises(ValueError, match='noise'):
                    modconv.synthesis_layer(x, weight, styles, bias, up, f, noise_const=bad, noise_strength=strength)
                with pytest.raises(ValueError, match='noise'):
                    if up == 1:
                        modconv.conv2d(x, wmod, noise=bad, noise_strength=strength)
                    else:
                        modconv.fir4_bias_act(y_t, f, bias, bad, strength, 'lrelu', 1.0, -1.0)
                if up == 2:
                    with pytest.raises(ValueError, match='noise'):
                        modconv.up2_fir(x, wmod, None, bias, bad, strength, 1, 1.0, -1.0)
                assert all(v == 0 for v in delta(c0).values()), (dtype, up, bad.shape, delta(c0))


def test_wide_torgb_fusion_declines_what_it_cannot_read(native):
    """conv3x3_torgb_wide_supported on device tensors: a skip image off a 16-byte boundary and a noise image of another size send the block to the two-launch form."""
    _lib, gradfix, modconv, *_ = _mods()
    n, ci, h = 3, 128, 128
    x = modconv.SplitActs(torch.zeros(n, ci, h, h, device='cuda').contiguous(memory_format=torch.channels_last))
    w, rgb_w, f = torch.zeros(128, ci, 3, 3, device='cuda'), torch.zeros(96, 128, 1, 1, device='cuda'), torch.ones(4, 4, device='cuda')
    prev = torch.zeros(n, 96, h // 2, h // 2, device='cuda')
    c0 = counters()
    with torch.no_grad():
        ok = lambda prev, noise=None: modconv.conv3x3_torgb_wide_supported(x, w, rgb_w, prev, f, 1, 'lrelu', noise=noise)
        assert ok(of.make('dense', prev, 'nhwc')) and ok(None) and ok(None, torch.zeros(h, h, device='cuda'))
        for form in ('offset1', 'offset8'):
            assert not ok(of.make(form, prev, 'nhwc')), form
        assert not ok(of.make('dense', prev, 'nchw'))
        for bad in (torch.zeros(h, h // 2, device='cuda'), torch.zeros(1, 1, h, h, device='cuda'), torch.zeros(h * h, device='cuda')):
            assert not ok(None, bad)
    assert all(v == 0 for v in delta(c0).values())


# ---- upfirdn2d and its gradient --------------------------------------------------------------------------------------------------------------------------------------------

UPFIRDN = {'up2': dict(up=2, padding=[2, 1, 2, 1], gain=4), 'down2': dict(down=2, padding=[1, 1, 1, 1]), 'fir4': dict(padding=[1, 1, 1, 1], gain=4)}


@functools.lru_cache(maxsize=None)
def _upfirdn_values(name, dt, vf):
    kw, dtype, vf = UPFIRDN[name], DTYPES[dt], dict(vf)
    g = torch.Generator().manual_seed(len(name))
    x = of.values(vf.get('x', 'dense'), torch.randn(2, 5, 37, 41, generator=g).to(dtype))
    from pix2pix3d_amd.torch_utils.ops import upfirdn2d
    f = of.values(vf.get('f', 'dense'), upfirdn2d.setup_filter([1, 3, 3, 1]))      # [4, 4]; 'expand': every row its first row — another filter, which the reference follows
    assert f.ndim == 2
    y = torch.from_numpy(np.ascontiguousarray(O.upfirdn2d(x.double().numpy(), f.double().numpy(), **kw))) if x.numel() else torch.zeros(0, 5, *_upfirdn_hw(kw, 37, 41, f), dtype=torch.float64)
    gy = of.values(vf.get('gy', 'dense'), torch.randn(y.shape, generator=g).to(dtype))
    gx = torch.from_numpy(np.ascontiguousarray(O.upfirdn2d_grad(gy.double().numpy(), tuple(x.shape), f.double().numpy(), **kw))) if x.numel() else torch.zeros(x.shape, dtype=torch.float64)
    return dict(x=x, f=f, gy=gy), dict(y=y, gx=gx)


def _upfirdn_hw(kw, h, w, f):
    up, down, p = kw.get('up', 1), kw.get('down', 1), kw['padding']
    return ((h * up + p[2] + p[3] - f.shape[0] + down) // down, (w * up + p[0] + p[1] - f.shape[1] + down) // down)


def _upfirdn_call(kw):
    from pix2pix3d_amd.torch_utils.ops import upfirdn2d

    def call(ops):
        x = ops['x'].requires_grad_(True)
        y = upfirdn2d.upfirdn2d(x, ops['f'], **kw)
        gx, = torch.autograd.grad(y, x, ops['gy']) if y.numel() else (torch.zeros_like(x),)
        return dict(y=y.detach(), gx=gx)
    return call


@functools.lru_cache(maxsize=None)
def _upfirdn_dense(name, dt, layout, vf):
    dense, ref = _upfirdn_values(name, dt, vf)
    return run_guarded(_upfirdn_call(UPFIRDN[name]), _device_operands(dense, {}, dict(x=layout, gy=layout)), ())


UPFIRDN_FORMS = [(lay, 'x', f) for lay in ('nchw', 'nhwc') for f in of.FORMS if f != 'unit'] + [('nhwc', 'f', f) for f in ('offset1', 'offset8', 'step', 'expand')] + \
                [('nhwc', 'gy', f) for f in ('offset1', 'batch_slice') + of.STRIDED_FORMS] + [('nchw', 'gy', 'offset1'), ('nchw', 'all', 'mixed'), ('nhwc', 'all', 'mixed')]


@pytest.mark.parametrize('layout,operand,form', UPFIRDN_FORMS)
@pytest.mark.parametrize('dt', list(DTYPES))
@pytest.mark.parametrize('name', list(UPFIRDN))
def test_upfirdn2d(native, name, dt, layout, operand, form):
    forms = dict(x='crop', f='step', gy='offset1') if operand == 'all' else {operand: form}
    if forms.get('x') == 'empty':
        forms['gy'] = 'dense'
    vf = vforms(forms)
    dense, ref = _upfirdn_values(name, dt, vf)
    dense_out, dense_d = _upfirdn_dense(name, dt, layout, vf)
    what = ('upfirdn2d', name, dt, layout, operand, form)
    out, d = run_guarded(_upfirdn_call(UPFIRDN[name]), _device_operands(dense, forms, dict(x=layout, gy=layout)), tuple(dense_out.values()))
    if form == 'empty':
        expect_route('none', d, dense_d, what)
        assert out['y'].shape == ref['y'].shape and out['y'].shape[0] == 0
        return
    assert d['upfirdn2d'] == dense_d['upfirdn2d'] == 2 and d['gradfix_aten'] == 0, (what, d, dense_d)      # one launch forward, one for the gradient, whatever the form
    # strides of the result follow x's memory format as the wrapper reads it (stride(1) == 1): compared with the dense call only for forms that keep it
    keeps_format = forms.get('x', 'dense') in ('dense',) + of.ALIGNMENT_FORMS and forms.get('gy', 'dense') in ('dense',) + of.ALIGNMENT_FORMS
    errs = {k: rel_err(out[k].double().cpu(), ref[k]) for k in ref}
    print(what, errs)
    for k in ref:
        assert out[k].shape == ref[k].shape and out[k].dtype == dense_out[k].dtype and (not keeps_format or out[k].stride() == dense_out[k].stride()), (what, k)
    assert all(e < UPFIRDN_TOL[DTYPES[dt]] for e in errs.values()), (what, errs)
    # (c) the counter is one per launch whichever kernel ran: a dense, aligned x takes the tiled / channels-last kernels, every other form of x or gy the generic
    # per-output kernel, which sums the same 16 products in another order — bit equality is not promised between them: a few fp32 ulps of the range (5e-7), or
    # one fp16 rounding step of the result (2^-10).  A filter in any form is read by strides by the SAME kernel: bit-identical
    if set(forms) == {'f'}:
        assert all(torch.equal(out[k], dense_out[k]) for k in ref), what
    else:
        bar = 5e-7 if DTYPES[dt] == torch.float32 else 2.0 ** -10
        assert all(rel_err(out[k].double().cpu(), dense_out[k].double().cpu()) < bar for k in ref), what


# ---- bias_act with first and second gradients ------------------------------------------------------------------------------------------------------------------------

BA_KW = dict(dim=1, act='lrelu', clamp=0.9)


@functools.lru_cache(maxsize=None)
def _bias_act_values(dt, vf):
    dtype, vf = DTYPES[dt], dict(vf)
    g = torch.Generator().manual_seed(3)
    mk = lambda k: of.values(vf.get(k, 'dense') if vf.get('x') not in ('empty', 'unit') else vf['x'], torch.randn(2, 16, 9, 21, generator=g).to(dtype))
    x, dy, ddx = mk('x'), mk('dy'), mk('ddx')
    b = torch.randn(16, generator=g).to(dtype)
    xs, bs, dys, ddxs = (t.double().numpy() for t in (x, b, dy, ddx))
    ref = dict(y=O.bias_act(xs, bs, **BA_KW))
    ref['dx'], ref['db'] = O.bias_act_grads(xs, bs, dys, **BA_KW)
    # lrelu has no second-order term in x: d(dx)/d(dy) applied to ddx is the first-order operator again
    ref['ddy'] = O.bias_act_grads(xs, bs, ddxs, **BA_KW)[0]
    return dict(x=x, b=b, dy=dy, ddx=ddx), {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ref.items()}


def _bias_act_call(ops):
    from pix2pix3d_amd.torch_utils.ops import bias_act
    x, b, dy = ops['x'].requires_grad_(True), ops['b'].requires_grad_(True), ops['dy'].requires_grad_(True)
    y = bias_act.bias_act(x, b, **BA_KW)
    if y.numel() == 0:
        return dict(y=y.detach())
    dx, db = torch.autograd.grad(y, [x, b], dy, create_graph=True)
    ddy, = torch.autograd.grad(dx, dy, ops['ddx'])
    return dict(y=y.detach(), dx=dx.detach(), db=db.detach(), ddy=ddy)


@functools.lru_cache(maxsize=None)
def _bias_act_dense(dt, layout, vf):
    dense, ref = _bias_act_values(dt, vf)
    return run_guarded(_bias_act_call, _device_operands(dense, {}, dict(x=layout, dy=layout, ddx=layout)), ())


BIAS_ACT_FORMS = [(lay, 'x', f) for lay in ('nchw', 'nhwc') for f in of.FORMS] + [('nhwc', k, f) for k in ('dy', 'ddx') for f in of.ALIGNMENT_FORMS[:2] + of.STRIDED_FORMS] + \
                 [('nchw', 'dy', 'offset1'), ('nchw', 'ddx', 'offset1'), ('nhwc', 'b', 'offset1'), ('nhwc', 'b', 'step'), ('nchw', 'all', 'mixed'), ('nhwc', 'all', 'mixed')]


@pytest.mark.parametrize('layout,operand,form', BIAS_ACT_FORMS)
@pytest.mark.parametrize('dt', list(DTYPES))
def test_bias_act(native, dt, layout, operand, form):
    forms = dict(x='offset1', b='step', dy='crop', ddx='offset8') if operand == 'all' else {operand: form}
    vf = vforms(forms)
    dense, ref = _bias_act_values(dt, vf)
    dense_out, dense_d = _bias_act_dense(dt, layout, vf)
    what = ('bias_act', dt, layout, operand, form)
    out, d = run_guarded(_bias_act_call, _device_operands(dense, forms, dict(x=layout, dy=layout, ddx=layout)), tuple(dense_out.values()))
    if form == 'empty':
        expect_route('none', d, dense_d, what)
        assert out['y'].shape == ref['y'].shape
        return
    assert d['bias_act'] == dense_d['bias_act'] >= 3, (what, d, dense_d)
    tol = BIAS_ACT_TOL[DTYPES[dt]]
    errs = {}
    for k in out:
        got, want = out[k].double().cpu().numpy(), ref[k].numpy()
        assert got.shape == want.shape, (what, k)
        diff = np.abs(got - want)
        if dt == 'f16' and k != 'db':                            # test_ops_gpu's rule: fp16 rounding can put a value on the other side of the kink or the clamp edge
            xs, bs = dense['x'].double().numpy(), dense['b'].double().numpy()
            if got.shape == xs.shape:
                yo = ref['y'].numpy()
                diff[(np.abs(np.abs(yo) - 0.9) < 5e-3) | (np.abs(xs + bs.reshape(1, -1, 1, 1)) < 5e-3)] = 0
        errs[k] = float(diff.max() / max(np.abs(want).max(), 1e-30))
    print(what, errs)
    # test_ops_gpu.test_bias_act_forward_and_gradients: y TOL, dx 2 TOL, db 4 TOL (fp32 only: an fp16 sum over 378 terms is not held there)
    assert errs['y'] < tol and errs['dx'] < 2 * tol and errs['ddy'] < 2 * tol and (dt == 'f16' or errs['db'] < 4 * tol), (what, errs)
    if forms.get('x', 'dense') in ('dense',) + of.ALIGNMENT_FORMS:
        for k in ('y', 'dx', 'ddy'):
            assert torch.equal(out[k], dense_out[k]), (what, k)     # element-wise: the scalar and the vector path give the same bits


# ---- the broadcast ops: a * b[n, c] + noise (fma.fma) and its reductions ----------------------------------------------------------------------------------------
# p3d_bcast_fma REFUSES x, y, z off a 16-byte boundary and reads the scales with scalar loads; p3d_channel_dot / p3d_pixel_sum REFUSE.  The dispatcher asks
# bcast.layout (dense, aligned, whole vectors) and the tensor-op formulation takes everything else.  A DEVIATION from the rule that alignment-only forms stay on
# the native kernels: bcast.py is left as it was, and an activation off its boundary is a 'fallback' row here.  The reason is byte counting, not a measurement:
# for an element-wise op a copy plus the kernel reads and writes the tensor twice, torch's own operators once or twice.

from test_bcast_gpu import SHAPES as BCAST_SHAPES      # noqa: E402

FMA_SHAPE = BCAST_SHAPES[0]
FMA_TOL = {torch.float32: (1e-6, 2e-5), torch.float16: (1e-3, 2e-3)}       # test_bcast_gpu (literals there): one rounding of the result; reductions accumulate in fp32
FMA_ROUTE = {   # (operand, form) -> launches of p3d_bcast_fma, p3d_channel_dot, p3d_pixel_sum in forward + backward; the dense call: (2, 1, 1)
    'native': (2, 1, 1), 'fallback': (0, 0, 0), 'backward_fallback': (1, 0, 0), 'none': (0, 0, 0)}
FMA_FORMS = [('a', f, 'native' if f == 'dense' else ('none' if f == 'empty' else 'fallback')) for f in of.FORMS if f not in ('unit', 'batch_slice')] + [('a', 'batch_slice', 'native')] + \
            [('b', 'offset1', 'native'), ('b', 'step', 'native'), ('b', 'expand', 'native'),                       # scales: copied to fp32 [N, C] or read by scalar loads
             ('z', 'offset1', 'fallback'), ('z', 'offset8', 'fallback'), ('z', 'crop', 'native'), ('z', 'expand', 'native'),      # a strided addend is copied (fresh, aligned); a dense one off its boundary is not
             ('gy', 'offset1', 'backward_fallback'), ('gy', 'offset8', 'backward_fallback'), ('gy', 'crop', 'native'), ('gy', 'expand', 'native'),
             ('all', 'mixed', 'fallback')]


@functools.lru_cache(maxsize=None)
def _fma_values(dt, shared, vf):
    dtype, vf = DTYPES[dt], dict(vf)
    n, c, h, w = FMA_SHAPE
    g = torch.Generator().manual_seed(c + w)
    a = of.values(vf.get('a', 'dense'), torch.randn(FMA_SHAPE, generator=g).to(dtype))
    b = of.values(vf.get('b', 'dense'), (torch.rand(n, c, 1, 1, generator=g) + 0.5).to(dtype))[:a.shape[0]]
    z = of.values(vf.get('z', 'dense'), torch.randn(1 if shared else n, 1, h, w, generator=g).to(dtype))
    z = z if shared else z[:a.shape[0]]
    gy = of.values(vf.get('gy', 'dense'), torch.randn(FMA_SHAPE, generator=g).to(dtype))[:a.shape[0]]
    ar, br, zr = (t.double().requires_grad_(True) for t in (a, b, z))
    yr = ar * br + zr
    if yr.numel():
        gar, gbr, gzr = torch.autograd.grad(yr, [ar, br, zr], gy.double())
    else:
        gar, gbr, gzr = torch.zeros_like(ar), torch.zeros_like(br), torch.zeros_like(zr)
    return dict(a=a, b=b, z=z, gy=gy), dict(y=yr.detach(), ga=gar, gb=gbr, gz=gzr)


def _fma_call(ops):
    from pix2pix3d_amd.torch_utils.ops import fma
    a, b, z = (ops[k].requires_grad_(True) for k in ('a', 'b', 'z'))
    y = fma.fma(a, b, z)
    if y.numel() == 0:
        return dict(y=y.detach())
    ga, gb, gz = torch.autograd.grad(y, [a, b, z], ops['gy'])
    return dict(y=y.detach(), ga=ga, gb=gb, gz=gz)


@pytest.mark.parametrize('operand,form,route', FMA_FORMS)
@pytest.mark.parametrize('shared', [True, False], ids=['shared_noise', 'noise_per_image'])
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_bcast_fma(native, dt, layout, shared, operand, form, route):
    from pix2pix3d_amd.torch_utils.ops import bcast
    forms = dict(a='offset1', b='expand', z='crop', gy='crop') if operand == 'all' else {operand: form}
    if shared and forms.get('z') == 'expand':
        forms['z'] = 'crop'                                      # (one shared image has no batch to expand)
    vf = vforms(forms)
    dense, ref = _fma_values(dt, shared, vf)
    what = ('fma', dt, layout, shared, operand, form)
    lay = dict(a=layout, gy=layout)
    runs = []
    for fm in ({}, forms):
        c0 = dict(bcast.calls)
        out, d = run_guarded(_fma_call, _device_operands(dense, fm, lay), ())
        runs.append((out, tuple(bcast.calls[k] - c0[k] for k in ('fma', 'dot', 'sum')), d))
    (dense_out, dense_calls, _), (out, calls, d) = runs
    assert dense_calls == (FMA_ROUTE['none'] if form == 'empty' else FMA_ROUTE['native']), (what, dense_calls)      # nothing aligned has moved off its kernel
    assert calls == FMA_ROUTE[route], (what, calls)
    if form == 'empty':
        assert launches(d) == 0 and out['y'].shape == ref['y'].shape
        return
    tol, rtol = FMA_TOL[DTYPES[dt]]
    errs = {k: rel_err(out[k].double().cpu(), ref[k]) for k in ref}
    print(what, errs)
    for k in ref:
        assert out[k].shape == ref[k].shape and out[k].dtype == dense_out[k].dtype, (what, k)
    assert errs['y'] < tol and errs['ga'] < tol and errs['gb'] < rtol and errs['gz'] < rtol, (what, errs)
    if calls == dense_calls:
        for k in ref:
            assert out[k].stride() == dense_out[k].stride() and torch.equal(out[k], dense_out[k]), (what, k)


# ---- scale channels (x * s[n, c]) and the bias sum: the other two entries of bcast.py, called as their callers call them ------------------------------------------------
# p3d_bcast_fma / p3d_channel_dot REFUSE tensors off a boundary; the scales are read by scalar loads.  Same deviation as above: what bcast.layout declines goes to
# the tensor-op formulation ('fallback'), which is what modulated_conv2d and bias_act's bias gradient write next to the call.

def _scale_call(ops):
    from pix2pix3d_amd.torch_utils.ops import bcast
    x, s = ops['x'].requires_grad_(True), ops['s'].requires_grad_(True)
    n, c = s.shape                                               # networks_stylegan2.modulated_conv2d
    y = bcast.scale_channels(x, s) if bcast.scale_channels_supported(x, s) else x * s.to(x.dtype).reshape(n, c, 1, 1)
    if y.numel() == 0:
        return dict(y=y.detach())
    gx, gs = torch.autograd.grad(y, [x, s], ops['gy'])
    return dict(y=y.detach(), gx=gx, gs=gs)


@functools.lru_cache(maxsize=None)
def _scale_values(dt, vf):
    dtype, vf = DTYPES[dt], dict(vf)
    n, c, h, w = FMA_SHAPE
    g = torch.Generator().manual_seed(n * c + h)
    x = of.values(vf.get('x', 'dense'), torch.randn(FMA_SHAPE, generator=g).to(dtype))
    s = of.values(vf.get('s', 'dense'), torch.randn(n, c, generator=g) + 1)[:x.shape[0]]
    gy = of.values(vf.get('gy', 'dense'), torch.randn(FMA_SHAPE, generator=g).to(dtype))[:x.shape[0]]
    xr, sr = x.double().requires_grad_(True), s.to(dtype).double().requires_grad_(True)
    yr = xr * sr.reshape(x.shape[0], c, 1, 1)
    gxr, gsr = torch.autograd.grad(yr, [xr, sr], gy.double()) if yr.numel() else (torch.zeros_like(xr), torch.zeros_like(sr))
    return dict(x=x, s=s, gy=gy), dict(y=yr.detach(), gx=gxr, gs=gsr)


SCALE_ROUTE = {'native': (2, 1), 'fallback': (0, 0), 'backward_fallback': (1, 0)}      # launches of p3d_bcast_fma, p3d_channel_dot in forward + backward
SCALE_FORMS = [('x', f, 'native' if f in ('dense', 'batch_slice') else 'fallback') for f in of.FORMS if f != 'unit'] + \
              [('s', 'offset1', 'native'), ('s', 'step', 'native'), ('s', 'expand', 'native'), ('s', 'ws_slice', 'native'),
               ('gy', 'offset1', 'backward_fallback'), ('gy', 'offset8', 'backward_fallback'), ('gy', 'crop', 'native'), ('gy', 'hw_swapped', 'native'), ('gy', 'expand', 'native'),
               ('all', 'mixed', 'fallback')]


@pytest.mark.parametrize('operand,form,route', SCALE_FORMS)
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_bcast_scale_channels(native, dt, layout, operand, form, route):
    from pix2pix3d_amd.torch_utils.ops import bcast
    forms = dict(x='offset8', s='step', gy='crop') if operand == 'all' else {operand: form}
    if forms.get('x') == 'empty':
        forms['gy'] = 'dense'
    vf = vforms(forms)
    dense, ref = _scale_values(dt, vf)
    what = ('scale_channels', dt, layout, operand, form)
    lay = dict(x=layout, gy=layout)
    runs = []
    for fm in ({}, forms):
        ops = _device_operands({k: v for k, v in dense.items() if k != 's'}, fm, lay)
        sd = dense['s'].cuda()
        ops['s'] = of.make_2d('ws_slice', sd) if fm.get('s') == 'ws_slice' else of.make(fm.get('s', 'dense'), sd)
        c0 = dict(bcast.calls)
        out, d = run_guarded(_scale_call, ops, ())
        runs.append((out, tuple(bcast.calls[k] - c0[k] for k in ('fma', 'dot')), d))
    (dense_out, dense_calls, _), (out, calls, d) = runs
    if form == 'empty':
        assert calls == (0, 0) and launches(d) == 0 and out['y'].shape == ref['y'].shape
        return
    assert dense_calls == SCALE_ROUTE['native'] and calls == SCALE_ROUTE[route], (what, dense_calls, calls)
    tol, rtol = FMA_TOL[DTYPES[dt]]
    errs = {k: rel_err(out[k].double().cpu(), ref[k]) for k in ref}
    print(what, errs)
    for k in ref:
        assert out[k].shape == ref[k].shape and out[k].dtype == dense_out[k].dtype, (what, k)
    assert errs['y'] < tol and errs['gx'] < tol and errs['gs'] < rtol, (what, errs)
    if calls == dense_calls:
        for k in ref:
            assert out[k].stride() == dense_out[k].stride() and torch.equal(out[k], dense_out[k]), (what, k)


def _bias_sum_call(ops):
    from pix2pix3d_amd.torch_utils.ops import bias_act
    t = ops['t'].requires_grad_(True)
    s = bias_act._sum_to_bias(t, 1)                              # bcast.bias_sum where bcast.bias_sum_supported, else t.sum([0, 2, 3]): bias_act's and conv2d_gradfix's call
    gt, = torch.autograd.grad(s, t, ops['gs'])
    return dict(s=s.detach(), gt=gt.clone())                     # (the gradient of a sum is an expanded VIEW of gs, here as in torch's own sum: not a result's own storage)


@pytest.mark.parametrize('operand,form,route', [('t', f, 'native' if f in ('dense', 'batch_slice') else 'fallback') for f in of.FORMS if f not in ('unit', 'empty')] +
                         [('gs', 'offset1', 'native'), ('gs', 'step', 'native'), ('all', 'mixed', 'fallback')])
@pytest.mark.parametrize('layout', ['nchw', 'nhwc'])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_bcast_bias_sum(native, dt, layout, operand, form, route):
    from pix2pix3d_amd.torch_utils.ops import bcast
    forms = dict(t='crop', gs='offset1') if operand == 'all' else {operand: form}
    dtype = DTYPES[dt]
    g = torch.Generator().manual_seed(11)
    t = of.values(forms.get('t', 'dense'), torch.randn(FMA_SHAPE, generator=g).to(dtype))
    gs = torch.randn(FMA_SHAPE[1], generator=g).to(dtype)
    ref = dict(s=t.double().sum([0, 2, 3]), gt=gs.double().reshape(1, -1, 1, 1).expand(t.shape))
    what = ('bias_sum', dt, layout, operand, form)
    runs = []
    for fm in ({}, forms):
        c0 = dict(bcast.calls)
        out, d = run_guarded(_bias_sum_call, _device_operands(dict(t=t, gs=gs), fm, dict(t=layout)), ())
        runs.append((out, bcast.calls['dot'] - c0['dot']))
    (dense_out, dense_calls), (out, calls) = runs
    assert dense_calls == 1 and calls == (1 if route == 'native' else 0), (what, dense_calls, calls)
    errs = {k: rel_err(out[k].double().cpu(), ref[k]) for k in ref}
    print(what, errs)
    assert out['s'].shape == ref['s'].shape and out['gt'].shape == t.shape and out['s'].dtype == dtype
    assert errs['s'] < FMA_TOL[dtype][1] and errs['gt'] == 0, (what, errs)                 # a reduction accumulated in fp32; its gradient is a broadcast
    if calls == dense_calls:
        assert torch.equal(out['s'], dense_out['s']), what


# ---- filtered_lrelu: the 2x2 case of test_filtered_lrelu_gpu, 5 channels at 37 x 41 ------------------------------------------------------------------------------------
# p3d_filtered_lrelu takes element strides for x and y and the bias stride, and loads element by element (no vector path, no alignment requirement): every form
# is 'native' — the same kernel, the same arithmetic, so bit-identical to the dense call.  The filters are rebuilt as fresh fp32 tables per call (_table).  The
# library refuses empty tensors; the wrapper answers N = 0 itself.

FL = dict(up=2, down=2, padding=[9, 10, 9, 10], gain=1.3, slope=0.2, clamp=0.9, flip_filter=False)
FL_TOL = {torch.float32: 2e-5, torch.float16: 4e-3}           # test_filtered_lrelu_gpu.test_forward_backward_match_reference_records (literals there); the gradient: 5 x


@functools.lru_cache(maxsize=None)
def _fl_values(dt, vf):
    from pix2pix3d_amd.torch_utils.ops import upfirdn2d
    dtype, vf = DTYPES[dt], dict(vf)
    g = torch.Generator().manual_seed(7)
    x = of.values(vf.get('x', 'dense'), torch.randn(2, 5, 37, 41, generator=g).to(dtype))
    b = torch.randn(5, generator=g).to(dtype)
    fu, fd = (upfirdn2d.setup_filter(torch.randn(12, generator=g).tolist()) for _ in range(2))
    kw = (FL['up'], FL['down'], FL['padding'], FL['gain'], FL['slope'])
    if x.numel() == 0:
        return dict(x=x, b=b, fu=fu, fd=fd, gy=x.new_zeros([0, 5, 36, 40])), dict(y=torch.zeros(0, 5, 36, 40, dtype=torch.float64))      # (2 * 37 + 19 - 22 + 1) // 2, (2 * 41 + 19 - 22 + 1) // 2
    xs, bs = x.double().numpy(), b.double().numpy()
    yo, so = O.filtered_lrelu(xs, fu.numpy(), fd.numpy(), bs, *kw, FL['clamp'], FL['flip_filter'], write_signs=True)
    gy = of.values(vf.get('gy', 'dense'), torch.randn(yo.shape, generator=g).to(dtype))
    gx = O.filtered_lrelu_backward(gy.double().numpy(), fu.numpy(), fd.numpy(), xs.shape, so, *kw, FL['flip_filter'])
    return dict(x=x, b=b, fu=fu, fd=fd, gy=gy), dict(y=torch.from_numpy(np.ascontiguousarray(yo)), gx=torch.from_numpy(np.ascontiguousarray(gx)))


def _fl_call(ops):
    from pix2pix3d_amd.torch_utils.ops import filtered_lrelu
    x = ops['x'].requires_grad_(True)
    y = filtered_lrelu.filtered_lrelu(x, fu=ops['fu'], fd=ops['fd'], b=ops['b'], **FL)
    gx, = torch.autograd.grad(y, x, ops['gy'])
    return dict(y=y.detach(), gx=gx)


@functools.lru_cache(maxsize=None)
def _fl_dense(dt, layout, vf):
    dense, ref = _fl_values(dt, vf)
    return run_guarded(_fl_call, _device_operands(dense, {}, dict(x=layout, gy=layout)), ())


FL_FORMS = [(lay, 'x', f) for lay in ('nchw', 'nhwc') for f in of.FORMS if f != 'unit'] + [('nhwc', 'b', 'offset1'), ('nhwc', 'b', 'step'), ('nhwc', 'fu', 'offset1'), ('nhwc', 'fd', 'step')] + \
           [('nhwc', 'gy', f) for f in ('offset1', 'offset8', 'crop', 'hw_swapped', 'expand')] + [('nchw', 'gy', 'offset1'), ('nchw', 'all', 'mixed'), ('nhwc', 'all', 'mixed')]


@pytest.mark.parametrize('layout,operand,form', FL_FORMS)
@pytest.mark.parametrize('dt', list(DTYPES))
def test_filtered_lrelu(native, dt, layout, operand, form):
    forms = dict(x='crop', b='step', fu='offset1', gy='offset1') if operand == 'all' else {operand: form}
    if forms.get('x') == 'empty':
        forms['gy'] = 'dense'
    vf = vforms(forms)
    dense, ref = _fl_values(dt, vf)
    dense_out, dense_d = _fl_dense(dt, layout, vf)
    what = ('filtered_lrelu', dt, layout, operand, form)
    out, d = run_guarded(_fl_call, _device_operands(dense, forms, dict(x=layout, gy=layout)), tuple(dense_out.values()))
    if form == 'empty':
        assert launches(d) == 0 and out['y'].shape == (0, 5, 36, 40) and out['gx'].shape == (0, 5, 37, 41), (what, d)
        return
    assert kernels_of(d) == kernels_of(dense_d) and d['filtered_lrelu'] == 2 and d['copies'] == 0, (what, d, dense_d)      # one launch forward, one for the gradient: 'native'
    tol = FL_TOL[DTYPES[dt]]
    errs = {k: rel_err(out[k].double().cpu(), ref[k]) for k in ref}
    print(what, errs)
    for k in ref:
        assert out[k].shape == ref[k].shape and out[k].dtype == dense_out[k].dtype, (what, k)
        assert torch.equal(out[k], dense_out[k]), (what, k, 'differs from the dense call on the same kernel')
    keeps_format = forms.get('x', 'dense') in ('dense',) + of.ALIGNMENT_FORMS and forms.get('gy', 'dense') in ('dense',) + of.ALIGNMENT_FORMS
    assert not keeps_format or all(out[k].stride() == dense_out[k].stride() for k in ref), what
    assert errs['y'] < tol and errs['gx'] < 5 * tol, (what, errs)


# ---- the fused ray-marcher: case 'seg' of render_cases at 8 + 8 samples, 64 rays per image ----------------------------------------------------------------------------
# p3d_render_forward checks no pointer's alignment.  Its kernels read rays, uniforms and limits element by element (a SCALAR path) and the packed decoder by
# 16-byte vectors — a fresh tensor the host fills (p3d_pack_decoder*, whose loads of the raw parameters are neither checked nor known to be scalar); the planes
# are read in place only where renderer._plane_set_cl finds channels-last strides of whole float4s from a 16-byte boundary, else re-laid into a fresh tensor
# (p3d_planes_to_channels_last, unchecked).  So the host guard comes first: every operand passes renderer._f32c = modconv.kernel_operand, and only that is run.
#   planes: dense [N,3,32,H,W] / offset / expand ..... 'copy+native' (re-layout launch, as the dense call)
#   planes: a channels-last backbone output [N,96,H,W] viewed [N,3,32,H,W] ..... 'native', read in place: one aux launch fewer; off its boundary: re-laid
#   rays as halves of one [N,M,6] tensor, expanded uniforms, decoder parameters as views into one flat buffer ..... 'copy+native'

from render_cases import load_case, make_decoder      # noqa: E402
from oracle import render_oracle as R                 # noqa: E402


@functools.lru_cache(maxsize=None)
def _render_scene(expand_planes, expand_uniforms):
    g, opts, dec_arrays = load_case('seg')
    opts = dict(opts, depth_resolution=8, depth_resolution_importance=8, ray_start=0.1, ray_end=0.5, box_warp=1, disparity_space_sampling=False, white_back=False)
    rng = np.random.RandomState(5)
    n, m = 2, 64
    planes = (0.5 * rng.randn(n, 3, 32, 8, 8)).astype(np.float32)
    o = np.zeros([n, m, 3], np.float32)
    o[..., 0], o[..., 1], o[..., 2] = rng.uniform(-0.4, 0.0, [n, m]), rng.uniform(-0.4, 0.0, [n, m]), -0.45
    d = np.tile(np.array([[[0.0, 0.0, 1.0]]], np.float32), [n, m, 1])
    uc, uf = rng.rand(n, m, 8).astype(np.float32), rng.rand(n * m, 8).astype(np.float32)
    if expand_planes:
        planes = np.repeat(planes[:1], n, 0)
    if expand_uniforms:
        uc, uf = np.repeat(uc[:1], n, 0), np.repeat(uf[:1], n * m, 0)
    ref = R.render(planes, dec_arrays, o, d, opts, uc, uf)
    return g, opts, dict(planes=planes, o=o, d=d, uc=uc, uf=uf), ref


def _flat_decoder(g):
    """The decoder with every parameter a view into ONE flat buffer, each at an odd offset (a flat parameter buffer of an optimizer or of data parallelism)."""
    dec = make_decoder(g, 'cuda')
    params = list(dec.parameters())
    flat = torch.full([sum(p.numel() + 1 for p in params) + 1], 7.0, device='cuda')
    at = 1
    for p in params:
        view = flat[at:at + p.numel()].view_as(p)
        view.copy_(p.data)
        p.data = view
        at += p.numel() + 1
    assert any(p.data_ptr() % 16 != 0 for p in params)
    return dec, flat


RENDER_FORMS = ['dense', 'planes_offset1', 'planes_offset8', 'planes_expand', 'planes_nchw96', 'planes_backbone_cl', 'planes_backbone_cl_offset1', 'rays_halves',
                'uniforms_expand', 'uniforms_offset1', 'decoder_flat', 'all']


@pytest.mark.parametrize('form', RENDER_FORMS)
def test_fused_render(native, form):
    from pix2pix3d_amd.training.volumetric_rendering import renderer
    g, opts, arrays, ref = _render_scene(form == 'planes_expand', form in ('uniforms_expand', 'all'))
    t = {k: torch.tensor(v, device='cuda') for k, v in arrays.items()}
    n, m = t['o'].shape[:2]

    def backbone_cl(planes, offset=False):                       # [N,96,H,W] channels-last, as the backbone hands it over, viewed as three planes of 32 channels
        img = of.make('offset1' if offset else 'dense', planes.reshape(n, 96, 8, 8), 'nhwc')
        return img.view(n, 3, 32, 8, 8)

    def operands(form):
        ops = dict(t)
        if form in ('planes_offset1', 'planes_offset8'):
            ops['planes'] = of.make(form[7:], t['planes'])
        elif form == 'planes_expand':
            ops['planes'] = of.make('expand', t['planes'])
        elif form == 'planes_nchw96':
            ops['planes'] = of.make('dense', t['planes'].reshape(n, 96, 8, 8), 'nchw').view(n, 3, 32, 8, 8)
        elif form in ('planes_backbone_cl', 'all'):
            ops['planes'] = backbone_cl(t['planes'])
        elif form == 'planes_backbone_cl_offset1':
            ops['planes'] = backbone_cl(t['planes'], offset=True)
        if form in ('rays_halves', 'all'):
            rays = torch.cat([t['o'], t['d']], -1)               # one [N, M, 6] tensor: the direction half starts 12 bytes in, rows of 24 bytes
            ops['o'], ops['d'] = rays[..., :3], rays[..., 3:]
        if form in ('uniforms_expand', 'all'):
            ops['uc'], ops['uf'] = of.make('expand', t['uc']), of.make('expand', t['uf'])
        if form == 'uniforms_offset1':
            ops['uc'], ops['uf'] = of.make('offset1', t['uc']), of.make('offset8', t['uf'])
        return ops

    def call(dec):
        def run(ops):
            out = renderer.fused_render(ops['planes'], dec, ops['o'], ops['d'], opts, ops['uc'], ops['uf'])
            assert out is not None
            return dict(zip(('feat', 'depth', 'wsum'), out))
        return run

    dec = make_decoder(g, 'cuda')
    dense_out, dense_d = run_guarded(call(dec), operands('dense'), ())
    flat = None
    if form in ('decoder_flat', 'all'):
        dec, flat = _flat_decoder(g)
        flat_before = flat.clone()
    out, d = run_guarded(call(dec), operands(form), tuple(dense_out.values()))
    assert flat is None or torch.equal(flat, flat_before)
    what = ('fused_render', form)
    assert dense_d['render'] == d['render'] >= 1 and d['gradfix_aten'] == 0, (what, d, dense_d)
    in_place = form in ('planes_backbone_cl', 'all')             # the re-layout launch is the one aux launch a plane set read in place saves
    assert d['aux'] == dense_d['aux'] - (1 if in_place else 0), (what, d, dense_d)
    if form in ('decoder_flat', 'uniforms_offset1', 'planes_offset1', 'planes_offset8', 'rays_halves', 'planes_backbone_cl_offset1', 'all'):
        assert d['copies'] > dense_d['copies'], (what, 'no copy was made', d, dense_d)
    e = (rel_err(out['feat'].cpu().numpy(), ref[0]), float(np.abs(out['depth'][..., 0].cpu().numpy() - ref[1]).max()), rel_err(out['wsum'][..., 0].cpu().numpy(), ref[2]))
    print(what, 'feat rel_err %.3g  depth abs %.3g  wsum rel_err %.3g' % e)
    assert e[0] < 2e-4 and e[1] < 5e-5 and e[2] < 2e-4, (what, e)      # tests/test_render_gpu.py's bounds against the numpy oracle (literals there)
    for k in dense_out:
        assert out[k].shape == dense_out[k].shape and out[k].dtype == dense_out[k].dtype and out[k].stride() == dense_out[k].stride(), (what, k)
        if form not in ('planes_expand', 'uniforms_expand', 'all'):      # the same values through the same kernel (in place or re-laid: the same texels)
            assert torch.equal(out[k], dense_out[k]), (what, k)
