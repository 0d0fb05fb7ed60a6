"""modconv.layer_route / torgb_route and the public predicates over them, against the answers the code gave BEFORE there was one route decision.

tests/golden/modconv_routes.npz was recorded from the commit before this refactor (883ba84) by a script that, per switch setting (``SWITCHES`` below) and case,
called that commit's ``_premod_route``, ``premodulate`` (its tag; the launches stubbed out), ``accepts_split_input``, ``is_small``, ``use_split_bf16``,
``use_shared_weights``, ``torgb_supported``, ``torgb_accumulates`` (with a matching fp32 NCHW ``out``) and ``premodulate_torgb`` (its tag) on stand-in tensors
like ``T`` below, and stored the answers as small integers (indices into ``KIND`` / ``TAGS``, 0 / 1 for the predicates).  Cases: 3x3 layers (n, ci, side, up,
dtype index) over batch (1, 2, 4, 8, 16, 17, 32) x channels (32, 48, 64, 128, 256, 512) x side (2 .. 256) x up (1, 2) x (fp16, fp32, bf16) = 2 016, plus every
conv0 / conv1 of every SynthesisBlock of seg2cat, seg2face and edge2car at batch 1, 4, 8 in the block's own dtype and in fp32 (``force_fp32``); ToRGB layers
(n, ci, co, side, dtype index, channels-last?) over a grid of 1 960 and every ToRGB of the same blocks."""
import numpy as np
import torch

from conftest import load_golden

DT = [torch.float16, torch.float32, torch.bfloat16]
KIND = ['gemm', 'shared', 'mfma']
SWITCHES = [{}, {'split_bf16': False}, {'split_activations': False}, {'shared_weight_max_pixels': 0}, {'gemm_max_pixels': 256}, {'gemm_max_pixels': 256, 'gemm_max_pixels_up': 256}]


class T:
    """Stand-in for a device tensor: shape, dtype and layout only."""
    is_cuda, requires_grad, ndim = True, False, 4

    def __init__(self, shape, dtype, nhwc=True):
        self.shape, self.dtype, self.nhwc = torch.Size(shape), dtype, nhwc

    def is_contiguous(self, memory_format=torch.contiguous_format):
        return (memory_format == torch.channels_last) == self.nhwc


def _switched(modconv, sw):
    saved = {k: getattr(modconv, k) for k in sw}
    for k, v in sw.items():
        setattr(modconv, k, v)
    return saved


def test_layer_route_gives_the_answers_of_the_five_statements_it_replaces():
    from pix2pix3d_amd.torch_utils.ops import modconv
    tags = [None, torch.float16, torch.float32, torch.bfloat16, modconv.BF16X3]
    g = load_golden('modconv_routes')
    cases, answers = g['conv_cases'].tolist(), g['conv_answers']
    assert len(cases) >= 2016 and answers.shape == (len(SWITCHES), len(cases), 7)
    for sw, want in zip(SWITCHES, answers.tolist()):
        saved = _switched(modconv, sw)
        try:
            for (n, ci, side, up, d), (route, tag_kind, tag_dtype, accepts, small, split, shared) in zip(cases, want):
                px, case = side * side, (sw, n, ci, side, up, DT[d])
                x, w, s = T([n, ci, side, side], DT[d]), T([ci, ci, 3, 3], torch.float32), T([n, ci], torch.float32)
                r = modconv.layer_route(n, ci, px, up, DT[d])
                assert r.kind == KIND[route], case                                                   # (the parent's _premod_route)
                assert r.tag == (KIND[tag_kind], up, tags[tag_dtype]), case                          # what premodulate labelled its product with
                # ... and what synthesis_layer compared it with, from the three predicates it combined
                assert r.kind == ('gemm' if small else ('shared' if split and shared else 'mfma')) and r.split == bool(split and not small), case
                assert r.tag[2] == (modconv.BF16X3 if split and not small else DT[d]), case
                assert bool(modconv.is_small(x, up)) == bool(small) and bool(modconv.use_split_bf16(x, ci)) == bool(split), case
                assert bool(modconv.use_shared_weights(x, w, s)) == bool(shared), case
                assert modconv.accepts_split_input(n, ci, px, up) == bool(accepts) == modconv.layer_route(n, ci, px, up, torch.float32).reads_split, case
                assert r.hands_split == bool(r.split and modconv.split_activations), case
        finally:
            _switched(modconv, saved)


def test_torgb_route_gives_the_answers_of_the_predicates_it_replaces():
    """One difference by design: where the route is the streaming kernel — it modulates in-kernel from the raw weights and styles — premodulate_torgb used to make
    fp32 weights that no consumer could match; now it makes nothing.  Those rows are exactly the ones ``streaming`` selects below (the condition is spelled out
    here, independently of the code under test); told that the block's conv1 fuses the ToRGB (``fused=True``), the fp32 weights that kernel reads are made as before."""
    from pix2pix3d_amd.torch_utils.ops import modconv
    tags = [None, torch.float16, torch.float32, torch.bfloat16, modconv.BF16X3]
    g = load_golden('modconv_routes')
    cases, answers = g['rgb_cases'].tolist(), g['rgb_answers']
    assert len(cases) >= 1960 and answers.shape == (len(SWITCHES), len(cases), 3)
    made = {}
    real = modconv.modulate_weights
    modconv.modulate_weights = lambda weight, styles, demodulate, dtype: made.setdefault('dtype', dtype)
    n_streaming = 0
    try:
        for sw, want in zip(SWITCHES, answers.tolist()):
            saved = _switched(modconv, sw)
            try:
                for (n, ci, co, side, d, nhwc), (supported, accumulates, pre_tag) in zip(cases, want):
                    case = (sw, n, ci, co, side, DT[d], nhwc)
                    x, w, s = T([n, ci, side, side], DT[d], bool(nhwc)), T([co, ci, 1, 1], torch.float32), T([n, ci], torch.float32)
                    out = T([n, co, side, side], torch.float32, False)
                    r = modconv.torgb_route(ci, co, side * side, DT[d], bool(nhwc))
                    assert bool(modconv.torgb_supported(x, w, s, True)) == bool(supported) == (r.kind is not None), case
                    assert bool(modconv.torgb_accumulates(x, w, out)) == bool(accumulates) == (r.kind == 'streaming'), case
                    streaming = DT[d] == torch.float16 and ci in (64, 128, 256) and co <= 32 and (side * side) % 4 == 0      # (premodulate_torgb assumes channels-last, as it did)
                    made.clear()
                    got = modconv.premodulate_torgb(w, s, side * side, DT[d])
                    if streaming:
                        n_streaming += 1
                        assert got is None and not made and tags[pre_tag] == torch.float32, case
                        assert modconv.premodulate_torgb(w, s, side * side, DT[d], fused=True)[1] == ('rgb', torch.float32) and made['dtype'] == torch.float32, case
                    else:
                        assert got[1] == ('rgb', tags[pre_tag]) and made['dtype'] == tags[pre_tag], case
            finally:
                _switched(modconv, saved)
    finally:
        modconv.modulate_weights = real
    assert n_streaming > 0
