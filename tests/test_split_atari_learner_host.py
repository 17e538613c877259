"""CPU-side checks of the Atari learner's opt-in split-bf16 convs (mzl_set_atari_precision; HipLearner(tower_precision=, stage_precision=)):
the switches' parsing and Python-side refusals, the header, and the data of tests/test_gpu_split_atari_learner.py -- a numpy model of a tile-path
conv in the split arithmetic (tests/split_atari_cases.py) equals the int64 conv over the whole plane on that data, every partial sum an exact
float32, and stops doing so under each planted mistake, so the GPU test's equality would catch the same mistake in a kernel."""
import os
import re

import numpy as np
import pytest

import conv_layer_cases as cc
import split_atari_cases as sa
from helpers import REPO


# ------------------------------------------------------------------------------------------ the switches
def test_atari_precisions_parse_like_conv_precision():
    from muzero_amd import hip_learner as hlm

    for which in ('tower_precision', 'stage_precision'):
        assert [hlm._atari_precision(v, which) for v in ('f32', 'bf16x3', 0, 1)] == [0, 1, 0, 1]
        for bad in ('bf16', 'F32', 2, -1, True, None, 1.5):
            with pytest.raises(ValueError, match=which):
                hlm._atari_precision(bad, which)


def test_constructor_refuses_unknown_values_before_touching_the_gpu():
    from muzero_amd.hip_learner import HipLearner

    for kw in (dict(tower_precision='bf16'), dict(stage_precision=2), dict(tower_precision='bf16x3', stage_precision='split')):
        with pytest.raises(ValueError, match='tower_precision|stage_precision'):
            HipLearner(None, 'cuda:0', 5, 4, lr=1e-3, **kw)


def test_make_hip_learner_passes_the_keywords_on():
    import inspect

    from muzero_amd import learner
    from muzero_amd.hip_learner import HipLearner

    for f in (learner.make_hip_learner, HipLearner.__init__):
        p = inspect.signature(f).parameters
        assert p['tower_precision'].default == 0 and p['stage_precision'].default == 0
    src = inspect.getsource(learner.make_hip_learner)
    assert 'tower_precision=tower_precision' in src and 'stage_precision=stage_precision' in src


def test_header_declares_the_setter_between_create_and_bind():
    from muzero_amd import hip_learner as hlm

    text = open(os.path.join(REPO, 'include', 'mzlearner.h')).read()
    assert re.search(r'int\s+mzl_set_atari_precision\(mz_learner\*\s*h,\s*int32_t\s+tower_precision,\s*int32_t\s+stage_precision\);', text)
    assert 'mzl_set_atari_precision' in hlm.ABI_SYMBOLS
    assert text.index('int mzl_create(') < text.index('int mzl_set_atari_precision(') < text.index('int mzl_bind(')
    assert 'mzl_debug_conv_tile' not in text  # (the hook is exported, not declared)


# ------------------------------------------------------------------------------------------ the model of the tile path
def test_tiles_are_cut_with_halo_and_zero_outside_the_plane():
    x = np.arange(1, 2 * 3 * 24 * 48 + 1, dtype=np.float32).reshape(2, 3, 24, 48)
    for wide, tw in ((True, 16), (False, 12)):
        t = sa.cut_tiles(x, sa.tile_w(48, wide))
        nty, ntx = 2, 48 // tw
        assert t.shape == (2 * nty * ntx, 3, 14, tw + 2)
        t = t.reshape(2, nty, ntx, 3, 14, tw + 2)
        assert np.array_equal(sa.put_tiles(t[..., 1:-1, 1:-1].reshape(-1, 3, 12, tw), 2, 24, 48, tw), x)  # the inner positions tile the plane
        assert not t[:, 0, :, :, 0].any() and not t[:, -1, :, :, -1].any() and not t[:, :, 0, :, :, 0].any() and not t[:, :, -1, :, :, -1].any()
        assert np.array_equal(t[:, 0, 1, :, 1:-1, 0], x[:, :, :12, tw - 1])      # a halo column inside the plane is the neighbour tile's edge
        assert np.array_equal(t[:, 1, 0, :, 0, 1:-1], x[:, :, 11, :tw])
    assert sa.tile_w(24) == 12 and sa.tile_w(48) == 16 and sa.tile_w(32) == 12 and sa.tile_w(96) == 16


RUNS = [(p, c, B, d) for p in sa.PLANES for c in sa.CHANNELS for B in sa.BATCHES for d in (0, 1)]
HOST_RUNS = [r for r in RUNS if r[2] == 1 or r[1] == (48, 24)]  # (every shape once, the partial-block layer at both batches: the model is slow numpy)


@pytest.mark.parametrize('plane,chan,B,direction', HOST_RUNS, ids=[f'{p}-{c[0]}to{c[1]}-n{B}-d{d}' for p, c, B, d in HOST_RUNS])
def test_integer_data_is_exact_and_the_model_equals_the_int64_conv(plane, chan, B, direction):
    for cls in sa.CLASSES:
        x, ws = sa.int_case(cls, plane, chan, B, direction)
        for w in ws:
            zero = np.zeros(w.shape[0], np.float32)
            plain, terms = cc.int_bounds(x, w, zero)
            assert plain < 1 << 23 and terms < 1 << 24, (cls, plain, terms)  # every partial sum of every order, term by term, an exact float32
            ref = cc.int_reference(x, w, zero)
            assert np.array_equal(sa.tile_conv_model(x, w, exact=True), ref), cls
            assert np.array_equal(sa.hook_weight(sa.hook_weight(w, direction), direction), w)


def test_the_locator_names_what_was_read_on_both_sides_of_every_seam():
    for plane, (H, W) in sa.PLANES.items():
        x, ws = sa.int_case('locator', plane, (16, 16), 2, 0)
        pos = sa.seam_positions(H, W)
        tw = sa.tile_w(W)
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (11, tw - 1), (11, tw), (12, tw - 1), (12, tw)} <= set(pos)
        ref = cc.int_reference(x, ws[0], np.zeros(16, np.float32))
        for co in range(16):
            tap, ci = co % 9, (7 * co) % 16
            for r, c in pos:
                rr, cq = r + tap // 3 - 1, c + tap % 3 - 1
                want = x[1, ci, rr, cq] if 0 <= rr < H and 0 <= cq < W else 0.0
                assert ref[1, co, r, c] == want  # a distinct code per (image, channel, position); 0 = the zero outside the plane
        assert len(np.unique(x)) == x.size and x.min() >= 1


# ------------------------------------------------------------------------------------------ mutation checks
def _model_fails(bug, plane, chan, B, direction):
    """True if some draw of some class separates the mutated model from the int64 conv."""
    for cls in sa.CLASSES:
        x, ws = sa.int_case(cls, plane, chan, B, direction)
        for w in ws:
            if not np.array_equal(sa.tile_conv_model(x, w, exact=True, bug=bug), cc.int_reference(x, w, np.zeros(w.shape[0], np.float32))):
                return True
    return False


@pytest.mark.parametrize('bug', sa.MUTATIONS)
def test_every_planted_mistake_breaks_the_integer_case(bug):
    # the partial-block mistake needs a layer that has one: 48 input channels forward, and the data gradient of a layer with 48 OUTPUT channels
    runs = [('p24', (48, 24), 1, 0), ('p48', (48, 24), 1, 0)] + ([] if bug == 'last_block' else [('p24', (16, 16), 2, 1), ('p48', (32, 32), 1, 1)])
    for run in runs:
        assert _model_fails(bug, *run), (bug, run)
    assert not _model_fails(None, 'p24', (48, 24), 1, 0)


def test_each_term_is_needed_by_a_class_of_its_own():
    """Dropping a term must fail on the class that NEEDS it (not by accident on another): W needs hh hm hl, X hh mh lh, M hh hm mh mm."""
    for cls, spec in cc.INT_CLASSES.items():
        x, ws = sa.int_case(cls, 'p24', (16, 16), 1, 0)
        for name in spec['needs']:
            assert any(not np.array_equal(sa.tile_conv_model(x, w, exact=True, bug='drop_' + name), cc.int_reference(x, w, np.zeros(16, np.float32))) for w in ws), (cls, name)
