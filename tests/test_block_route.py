"""modconv.block_route on the CPU, against what the commit before it did on an MI355X (tests/golden/block_routes.json, tests/block_trace.py): for every block of
every recorded case the route, evaluated from the block record's numbers alone, names the form whose launch wrapper the recording shows for that block."""
import pytest
import torch

import block_trace as T

# form -> the wrapper its ToRGB goes through (RGB_WIDE_ADD and RGB_LAYER both run the ToRGB layer, whose native route is modconv.torgb)
WRAPPER = {'conv_wide_skip': 'conv3x3_torgb_wide', 'wide_skip': 'torgb_wide_skip', 'wide_add': 'torgb', 'fused': 'conv3x3_torgb', 'fused_dead': 'conv3x3_torgb', 'layer': 'torgb'}
DTYPE = {'float16': torch.float16, 'float32': torch.float32}
# the two cases whose last backbone block is handed a skip image its first form's operand check refuses: the recording shows a LATER form of the route's list
FALLS = {'seg2cat-b4-skip-image-strided': 'layer', 'seg2cat-b4-skip-image-offset4': 'wide_add'}


def blocks_of(events):
    """[(block record, [wrapper names called before the next block began], [shapes of the SplitActs made by then])]"""
    out = []
    for ev in events:
        if ev[0] == 'block':
            out.append((ev[1], [], []))
        elif ev[0] == 'wrapper':
            out[-1][1].append(ev[1])
        elif ev[0] == 'split' and out:
            out[-1][2].append(ev[1])
    return out


def route_of(modconv, b):
    return modconv.block_route(b['batch'], b['in_channels'], b['out_channels'], b['img_channels'], b['resolution'], b['in_div'], DTYPE[b['dtype']], b['channels_last'],
                               b['architecture'], b['is_last'], b['fused_modconv'], b['noise_mode'], b['use_noise'], b['activation'], b['has_img'], b['split_ok'], b['x_dead'])


def test_the_recording_covers_the_cases_and_every_form():
    rec = T.load_recording()
    assert set(rec['cases']) == set(T.cases())
    seen = {name for case in rec['cases'] for _, names, _ in blocks_of(T.recorded_events(rec, case)) for name in names}
    assert seen == set(T.WRAPPERS)
    for case_id, case in T.cases().items():
        unstable = set(rec['cases'][case_id]['unstable'])
        assert case['noise_mode'] == 'random' or not unstable & {'image_raw', 'image_depth'}
        assert set(rec['cases'][case_id]['digests']) == set(T.OUTPUTS) - unstable


def planned_modulations(modconv, b, route):
    """The p3d_modulate_weights calls (from ``dtype`` on) the plan issues ahead for a block, read off its BlockRoute: a per-image ('mfma') layer's weights in its
    tag's dtype — a shared-weight layer gets demodulation coefficients instead —, the ToRGB's in rgb_route.pre_tag's where that is one."""
    from pix2pix3d_amd import _lib
    code = lambda dt: modconv.DTYPE_F32_BF16X3 if dt == modconv.BF16X3 else _lib.DTYPE_CODE[dt]
    n, ci, co = b['batch'], b['in_channels'], b['out_channels']
    out = [[code(r.tag[2]), n, co, cin, 9, 1, 1.0, 0] for r, cin in ((route.conv0, ci), (route.conv1, co)) if r is not None and r.kind == 'mfma']
    if route.rgb and route.rgb_route.pre_tag is not None and modconv.premodulate_rgb:
        out.append([code(route.rgb_route.pre_tag[1]), n, b['img_channels'], co, 1, 0, 1.0, 0])
    return out


def test_an_orig_backbones_last_block_is_handed_no_image_and_plans_no_torgb_product():
    """architecture='orig': only the last block has a ToRGB and no skip image reaches it, so its fp16 ToRGB runs the streaming kernel, which takes no product from
    the plan; a head's block of the same sizes IS handed an image and fuses the ToRGB into conv1, which takes one."""
    from pix2pix3d_amd.torch_utils.ops import modconv
    args = (1, 256, 128, 3, 256, 2, torch.float16, True, 'orig', True, True, 'none', True, 'lrelu')
    backbone, head = modconv.block_route(*args, has_img=False), modconv.block_route(*args, has_img=True)
    assert backbone.rgb == ('layer',) and backbone.rgb_route.kind == 'streaming' and backbone.rgb_route.pre_tag is None and not backbone.img_first
    assert head.rgb == ('fused', 'layer') and head.rgb_route.kind == 'fused' and head.rgb_route.pre_tag == ('rgb', torch.float32) and head.img_first


@pytest.mark.parametrize('case_id', list(T.cases()))
def test_block_route_names_the_form_the_parent_took(case_id):
    from pix2pix3d_amd.torch_utils.ops import modconv
    rec, case = T.load_recording(), T.cases()[case_id]
    name = case.get('switch')
    saved = getattr(modconv, name) if name else None
    if name:
        setattr(modconv, name, 0 if name == 'shared_weight_max_pixels' else not saved)
    try:
        fell, planned = [], []
        for b, wrappers, splits in blocks_of(T.recorded_events(rec, case_id)):
            route = route_of(modconv, b)
            assert len(wrappers) == (1 if route.rgb else 0), (b, route.rgb, wrappers)
            if route.rgb and wrappers != [WRAPPER[route.rgb[0]]]:
                fell.append(b)
                later = FALLS[case_id]                          # (KeyError: a case that may not differ)
                assert later in route.rgb[1:] and wrappers == [WRAPPER[later]], (b, route.rgb, wrappers)
            # SplitActs are made where the route says so and nowhere else: by conv1 (a plain 3x3 launch always grants it) unless the launch that ran it stored no
            # activations at all, and by conv0 where the x2 kernel that ended up producing its result could (LayerRoute.hands_split: "may", not "will")
            by_conv1 = int(route.split and route.conv1.hands_split and wrappers != ['conv3x3_torgb_wide'])
            assert by_conv1 <= len(splits) <= by_conv1 + int(route.split and route.conv0.hands_split), (b, route, splits)
            assert all(shape == [b['batch'], b['out_channels'], b['resolution'], b['resolution']] for shape in splits), (b, splits)
            planned += planned_modulations(modconv, b, route) if modconv.prefetch_styles else []
        assert len(fell) == (1 if case_id in FALLS else 0)
        # what the plan made ahead on the prefetch stream is what the routes' tags name (conv0, conv1: LayerRoute.tag; the ToRGB: rgb_route.pre_tag), product for product
        ahead = [ev[3][3:] for ev in T.recorded_events(rec, case_id) if ev[:3] == ['call', 'p3d_modulate_weights', 'side']]
        assert T.arg_names('p3d_modulate_weights')[3:] == ['dtype', 'n_img', 'co', 'ci', 'taps', 'demodulate', 'pre_scale', 'oihw_order']
        assert sorted(ahead) == sorted(planned), case_id
    finally:
        if name:
            setattr(modconv, name, saved)
