"""The forms a caller's tensor can take: ``make(form, dense, layout)`` returns a tensor with the values and the logical shape of ``dense`` (a dense CPU or
device tensor), held as ``form`` says.  Device tests feed every native op such operands (test_operand_forms_gpu.py); test_operand_forms_host.py checks that
each form has the property it promises.  A plain helper module, like render_cases.py."""
import torch

# alignment only: dense in the asked layout, first element off a 16-byte boundary
ALIGNMENT_FORMS = ('offset1', 'offset8', 'batch_slice')
# strided: not dense in any layout a kernel reads
STRIDED_FORMS = ('chan_slice', 'crop', 'step', 'hw_swapped', 'expand')
FORMS = ('dense',) + ALIGNMENT_FORMS + STRIDED_FORMS + ('empty', 'unit')
FORMS_4D_ONLY = ('chan_slice', 'crop', 'hw_swapped')
FORMS_2D_ONLY = ('transposed', 'ws_slice')                   # make_2d: a matrix as the .t() of a dense one; rows as ws[:, k] of a dense [N, K, F]


def fmt_of(layout):
    return torch.channels_last if layout == 'nhwc' else torch.contiguous_format


def _dense(t, layout):
    """A fresh copy of ``t`` in ``layout`` (4-D) or contiguous (any other rank); fresh allocations start on a 16-byte boundary."""
    if t.ndim == 4 and layout == 'nhwc':
        return torch.empty_like(t, memory_format=torch.channels_last).copy_(t)
    return torch.empty_like(t, memory_format=torch.contiguous_format).copy_(t)


def _phys(t, layout):
    """(shape as the memory order has it, the permutation from it back to the logical order)."""
    if t.ndim == 4 and layout == 'nhwc':
        n, c, h, w = t.shape
        return (n, h, w, c), (0, 3, 1, 2)
    return tuple(t.shape), tuple(range(t.ndim))


def _at_offset(t, layout, elems):
    """``t`` dense in ``layout`` inside a flat buffer, ``elems`` elements past its (aligned) start."""
    shape, back = _phys(t, layout)
    flat = torch.empty([t.numel() + elems + 16], dtype=t.dtype, device=t.device).fill_(7)
    view = flat[elems:elems + t.numel()].view(shape).permute(back)
    view.copy_(t)
    return view


def make(form, dense, layout='nchw'):
    """``dense`` held as ``form``; ``layout`` ('nchw' / 'nhwc') applies to 4-D tensors.  The result never shares memory with ``dense``.
    'expand': the values are those of ``dense[:1]`` repeated (the caller's reference takes ``values(form, dense)``).  'empty': ``dense[:0]``.
    'unit': H = W = 1 cut out of a larger tensor (4-D; dim 0 of length 1 for other ranks) — the values of ``dense[..., :1, :1]``."""
    t = dense.detach()
    assert form in FORMS and (t.ndim == 4 or form not in FORMS_4D_ONLY)
    item = t.element_size()
    if form == 'dense':
        return _dense(t, layout)
    if form == 'offset1':
        return _at_offset(t, layout, 1)
    if form == 'offset8':
        assert 8 % item == 0
        return _at_offset(t, layout, 8 // item)
    if form == 'batch_slice':                                # bigger[1:1+N]: off a boundary when one image is no multiple of 16 bytes
        big = _dense(torch.cat([t[:1] * 0 + 7, t, t[:1] * 0 + 7]), layout)
        return big[1:1 + t.shape[0]]
    if form == 'chan_slice':                                 # wider[:, 3:3+C]
        pad_l, pad_r = t[:, :1].expand(-1, 3, -1, -1) * 0 + 7, t[:, :1].expand(-1, 2, -1, -1) * 0 + 7
        return _dense(torch.cat([pad_l, t, pad_r], 1), layout)[:, 3:3 + t.shape[1]]
    if form == 'crop':                                       # larger[:, :, 1:1+H, 2:2+W]
        n, c, h, w = t.shape
        big = _dense(t.new_full([n, c, h + 2, w + 5], 7), layout)
        big[:, :, 1:1 + h, 2:2 + w] = t
        return big[:, :, 1:1 + h, 2:2 + w]
    if form == 'step':                                       # doubled[..., ::2]
        big = _dense(t.new_full([*t.shape[:-1], 2 * t.shape[-1]], 7), layout)
        big[..., ::2] = t
        return big[..., ::2]
    if form == 'hw_swapped':                                 # .transpose(2, 3) of a dense [N, C, W, H]
        return _dense(t.transpose(2, 3), layout).transpose(2, 3)
    if form == 'expand':                                     # stride 0 along dim 0
        return _dense(t[:1], layout).expand(t.shape[0], *[-1] * (t.ndim - 1))
    if form == 'empty':
        return _dense(t[:0], layout)
    if form == 'unit':
        if t.ndim == 4:
            n, c, h, w = t.shape
            big = _dense(t.new_full([n, c, 3, 4], 7), layout)
            big[:, :, 1:2, 2:3] = t[:, :, :1, :1]
            return big[:, :, 1:2, 2:3]
        big = _dense(torch.cat([t[:1] * 0 + 7, t[:1], t[:1] * 0 + 7]), layout)
        return big[1:2]
    raise AssertionError(form)


def make_2d(form, dense):
    """The two forms only a matrix has.  'transposed': ``.t()`` of a dense [W, H] (dense, column-major).  'ws_slice': ``ws[:, 1]`` of a dense [N, 3, F] — rows
    at a stride of 3 F elements, each contiguous (a layer's latent as the synthesis network hands it over)."""
    t = dense.detach()
    assert t.ndim == 2 and form in FORMS_2D_ONLY
    if form == 'transposed':
        return _dense(t.t(), 'nchw').t()
    ws = t.new_full([t.shape[0], 3, t.shape[1]], 7)
    ws[:, 1] = t
    return ws[:, 1]


def kernel_ready(shape, strides, address, fmt=torch.contiguous_format):
    """What modconv.kernel_operand promises, written out as a function of shape, element strides and the byte address of the first element: the tensor is dense
    in ``fmt`` (torch's own rule: the stride of a size-1 dimension counts for nothing) and starts on a 16-byte boundary; an empty tensor is never read."""
    if 0 in shape:
        return True
    order = (1, 3, 2, 0) if fmt == torch.channels_last else range(len(shape) - 1, -1, -1)
    expect = 1
    for d in order:
        if shape[d] != 1 and strides[d] != expect:
            return False
        expect *= shape[d]
    return address % 16 == 0



def values(form, dense):
    """The values ``make(form, dense, ...)`` holds, as a dense tensor (what a reference computes on)."""
    t = dense.detach()
    if form == 'expand':
        return t[:1].expand(t.shape[0], *[-1] * (t.ndim - 1)).clone()
    if form == 'empty':
        return t[:0].clone()
    if form == 'unit':
        return (t[:, :, :1, :1] if t.ndim == 4 else t[:1]).clone()
    return t.clone()


def base_of(t):
    """The whole buffer ``t`` is a view of, as a flat tensor: compared before and after a call, it shows a write past the view."""
    return torch.empty([0], dtype=t.dtype, device=t.device).set_(t.untyped_storage())


def shares_storage(a, b):
    return a.numel() > 0 and b.numel() > 0 and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
