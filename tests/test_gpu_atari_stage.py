"""The Atari representation's launches outside its stride-1 convs, ONE launch group at a time through mzl_debug_atari_stage -- the AtariRun members the
update itself calls (s2_fwd, s2_dgrad, pool_fwd, pool_bwd, relu_bwd, entry, entry12, gather, scatter) and launch_entry / launch_normalize -- on the
data of tests/atari_stage_cases.py, where equality with an int64 / float64 / float32-expression reference is the assertion (and, for the two inexact
entry classes, a derived bound per element).  tests/test_atari_stage_host.py shows on the CPU that this data tells every planted mistake from the
reference.

Handles: a small Atari learner, one created under MZLC_NO_TAPSETS=1 (nine-tap parity copies), one under MZLC_NO_WIDE_TILES=1 (12 x 12 tiles at every
width), and board learners of 3 x 3 and 15 x 15 for launch_entry.  The conv learner refuses boards above 240 points, so a 19 x 19 handle -- whose
launch_entry would walk 12 chunks on 8 workgroups -- cannot exist: test_boards_above_240_points_have_no_conv_learner pins that; the chunk loop with its
barriers runs in AtariRun::entry at hw = 2304 (72 chunks on 64 workgroups)."""
import os

import numpy as np
import pytest
import torch

import atari_stage_cases as ac
from helpers import build_conv, conv_case

pytestmark = pytest.mark.gpu
PARITIES = ((0, 0), (0, 1), (1, 0), (1, 1))
MZL_E_INVALID = -1  # include/mzlearner.h


def _learner(case, env=None, max_batch=2):
    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    net = build_conv(case).to(dev)
    net.train()
    if env:
        assert env not in os.environ
        os.environ[env] = '1'
    try:
        return HipLearner(net, dev, 1, max_batch, lr=1e-3)
    finally:
        if env:
            del os.environ[env]


@pytest.fixture(scope='module')
def atari():
    hl = _learner(conv_case('atari_s'))
    yield hl
    hl.close()


@pytest.fixture(scope='module')
def nine_tap():
    hl = _learner(conv_case('atari_s'), 'MZLC_NO_TAPSETS')
    yield hl
    hl.close()


@pytest.fixture(scope='module')
def narrow():
    hl = _learner(conv_case('atari_s'), 'MZLC_NO_WIDE_TILES')
    yield hl
    hl.close()


BOARDS = {'board3': conv_case('board3'), 'board15': ('board15', 'board', (5, 15, 15), 226, 1, 24, 1, 1, 31)}


@pytest.fixture(scope='module')
def boards():
    hls = {name: _learner(case) for name, case in BOARDS.items()}
    yield hls
    for hl in hls.values():
        hl.close()


def _same(out, ref, what=''):
    """Bit equality of two float32 arrays (NaN-free reference), with the first difference spelled out."""
    out, ref = np.asarray(out), np.asarray(ref, np.float32)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert not np.isnan(out).any(), f'{what}: {int(np.isnan(out).sum())} elements were never written'
    bad = np.argwhere(out != ref)
    assert len(bad) == 0, f'{what}: {len(bad)} values differ, first at {bad[0].tolist()}: {out[tuple(bad[0])]} != {ref[tuple(bad[0])]}'


# ------------------------------------------------------------------------------------------ stride-2 forward conv
def _masks(name):
    return tuple(int(m, 16) for m in name.split('masks=')[1].split(','))


@pytest.mark.parametrize('shape', ac.S2_FWD, ids=str)
def test_s2_fwd_equals_the_int64_conv(atari, nine_tap, narrow, shape):
    cin, cout, H, W, B = shape
    for cls in ac.S2_CLASSES:
        x, ws = ac.s2_case(cls, shape)
        for w in ws:
            ref = ac.s2_direct(x, w).astype(np.float32)
            y, name = atari.debug_atari_stage('s2_fwd', weight=w, x=x)
            _same(y, ref, f'{cls} {name}')
            assert _masks(name) == (0x010, 0x018, 0x012, 0x01b) and ' compact=1 ' in name
            assert ('NPT=16 tile=12x16' if W == 48 else 'NPT=13 tile=12x12') in name, name
            y9, name9 = nine_tap.debug_atari_stage('s2_fwd', weight=w, x=x)
            _same(y9, ref, f'{cls} {name9}')
            assert _masks(name9) == (0x1ff,) * 4 and ' compact=0 ' in name9
            if W == 48:  # the same plane as 12 x 12 tiles
                yn, namen = narrow.debug_atari_stage('s2_fwd', weight=w, x=x)
                _same(yn, ref, f'{cls} {namen}')
                assert 'NPT=13 tile=12x12' in namen


# ------------------------------------------------------------------------------------------ stride-2 data gradient
@pytest.mark.parametrize('shape', ac.S2_DGRAD, ids=str)
def test_s2_dgrad_equals_the_int64_data_gradient(atari, nine_tap, shape):
    for cls in ac.S2_CLASSES:
        dy, ws = ac.s2_case(cls, shape, dgrad=True)
        for w in ws:
            ref = ac.s2_dgrad_direct(dy, w).astype(np.float32)
            for hl in (atari, nine_tap):
                dx, name = hl.debug_atari_stage('s2_dgrad', weight=w, dy=dy)
                _same(dx, ref, f'{cls} {name}')  # (NaN preset + equality on all of the 48 x 48 plane: each parity was written, and once)
            assert _masks(name) == (0x1ff,) * 4


def test_s2_dgrad_on_wide_tiles_is_refused_in_the_compact_form_and_exact_in_the_nine_tap_form(atari, nine_tap, narrow):
    from muzero_amd.hip_learner import LearnerError

    for cls in ac.S2_CLASSES:
        dy, ws = ac.s2_case(cls, ac.S2_DGRAD_WIDE, dgrad=True)
        ref = ac.s2_dgrad_direct(dy, ws[0]).astype(np.float32)
        with pytest.raises(LearnerError, match=r'no kernel build: kConvBuilds has none for NPT=16 \(tile 12x16\) and the data-gradient tap sets'):
            atari.debug_atari_stage('s2_dgrad', weight=ws[0], dy=dy)
        dx, name = nine_tap.debug_atari_stage('s2_dgrad', weight=ws[0], dy=dy)
        _same(dx, ref, f'{cls} {name}')
        assert 'NPT=16 tile=12x16' in name
        dx, name = narrow.debug_atari_stage('s2_dgrad', weight=ws[0], dy=dy)  # 12 x 12 tiles: the compact data-gradient tap sets are built
        _same(dx, ref, f'{cls} {name}')
        assert _masks(name) == (0x010, 0x030, 0x090, 0x1b0)
    # the refused call left the handle as it was
    x, ws = ac.s2_case('small', ac.S2_FWD[0])
    _same(atari.debug_atari_stage('s2_fwd', weight=ws[0], x=x)[0], ac.s2_direct(x, ws[0]), 'after the refusal')


# ------------------------------------------------------------------------------------------ pools, ReLU backward
@pytest.mark.parametrize('hw', ac.POOLS, ids=str)
def test_pools_equal_the_float32_quotient_of_the_int64_window_sum(atari, hw):
    x, g = ac.pool_case(hw)
    y, name = atari.debug_atari_stage('pool_fwd', x=x)
    assert np.array_equal(y.view(np.uint32), ac.pool_fwd_ref(x).view(np.uint32)), name
    gin, name = atari.debug_atari_stage('pool_bwd', g=g)
    assert gin.shape == x.shape and np.array_equal(gin.view(np.uint32), ac.pool_bwd_ref(g).view(np.uint32)), name


def test_relu_bwd_bits(atari):
    g, x = ac.relu_case()
    dz, name = atari.debug_atari_stage('relu_bwd', g=g, x=x)
    assert np.array_equal(dz.view(np.uint32), ac.relu_bwd_ref(g, x).view(np.uint32)), name


# ------------------------------------------------------------------------------------------ entry
def _groups_rule(launcher, B, hw, plain):
    if launcher == 'atari':
        return B * min(-(-(hw // 4) // 32), 32) if plain else B * min(-(-hw // 32), 64)
    return B * min(-(-hw // 32), 8)  # ENTRY_SPLIT


def _check_entry(hl, launcher, cls, B, C, hw_shape, scale, use_gs, use_extra, key=0):
    n = hw_shape[0] * hw_shape[1]
    case = ac.entry_case(cls, B, C, n, key)
    shp = (B, C) + hw_shape
    gs, extra = (case['gs'] if use_gs else None), (case['extra'] if use_extra else None)
    kw = dict(x=case['x'].reshape(shp), partner=case['partner'].reshape(shp), scale=scale, launcher=launcher)
    if use_gs:
        kw['gs'] = gs.reshape(shp)
    if use_extra:
        kw['extra'] = extra.reshape(shp)
    dz, name, part = hl.debug_atari_stage('entry', **kw)
    what = f'{launcher} {cls} B={B} C={C} hw={n} scale={scale} gs={use_gs} extra={use_extra}: {name}'
    plain = launcher == 'atari' and not use_gs and use_extra and n % 4 == 0
    assert ('k_lc_entry_plain' in name) == plain, what
    assert part.shape[0] == _groups_rule(launcher, B, n, plain), what
    ref = ac.entry_ref(case['x'], gs, scale, extra, case['partner'])
    dz = dz.reshape(B, C, n)
    assert not np.isnan(dz).any(), what
    exact = cls in ac.EXACT_CLASSES or not use_gs  # (without gs, dz = extra [x > 0]: exact on any data)
    if exact:
        if use_gs:  # the precondition of equality, on THIS data: d exact, every term dyadic, every sum of absolute values under 2^24
            d_exact, dyadic, top = ac.entry_exactness(case, scale, use_extra)
            assert d_exact and dyadic and top < 1 << 24, (what, top)
        assert np.array_equal(ref['dz'].astype(np.float32).astype(np.float64), ref['dz'])
        _same(dz, ref['dz'], what)
    else:
        if cls == 'flat':
            zero = (case['x'] == 0).all(1, keepdims=True) & np.ones((1, C, 1), bool)
            assert zero.any() and not dz[zero].any(), what
        bound = ac.entry_bound(ref, extra)
        err = np.abs(dz.astype(np.float64) - ref['dz'])
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        assert (err <= bound).all(), f'{what}: |got - ref| = {err[worst]} > {bound[worst]} at {worst}'
    if cls in ac.EXACT_CLASSES:
        p = part.reshape(B, -1, part.shape[1], 2)[:, :, :C].astype(np.float64)
        assert np.isfinite(p).all(), what
        assert np.array_equal(p[..., 0].sum(1), ref['sum1']) and np.array_equal(p[..., 1].sum(1), ref['sum2']), what


# (B, scale, gs, extra): every B x scale x extra with gs, and per B the gs-null call, which reaches k_lc_entry_plain in AtariRun::entry
COMBOS = tuple((B, scale, True, extra) for B in (1, 3) for scale in (0.5, 1.0) for extra in (True, False)) + ((1, 1.0, False, True), (3, 1.0, False, True))


@pytest.mark.parametrize('hw', sorted(ac.ENTRY_HW))
@pytest.mark.parametrize('C', ac.ENTRY_C)
def test_entry_through_AtariRun_entry(atari, C, hw):
    for cls in ac.ENTRY_CLASSES:
        for B, scale, use_gs, use_extra in COMBOS:
            _check_entry(atari, 'atari', cls, B, C, ac.ENTRY_HW[hw], scale, use_gs, use_extra)


@pytest.mark.parametrize('C', ac.ENTRY_C)
def test_entry_of_the_12x12_stage(atari, C):
    for cls in ac.ENTRY_CLASSES:
        for B in (1, 3):
            _check_entry(atari, 'rep12', cls, B, C, (12, 12), 1.0, False, True)


@pytest.mark.parametrize('board', sorted(BOARDS))
def test_entry_through_launch_entry_on_board_handles(boards, board):
    case = BOARDS[board]
    C, hw_shape = case[5], case[2][1:]
    for cls in ac.ENTRY_CLASSES:
        for B, scale, use_gs, use_extra in COMBOS:
            _check_entry(boards[board], 'tower', cls, B, C, hw_shape, scale, use_gs, use_extra)
    # (and AtariRun::entry takes a board handle too)
    _check_entry(boards[board], 'atari', 'ties', 3, 13, (6, 6), 0.5, True, True)


def test_boards_above_240_points_have_no_conv_learner():
    """launch_entry cuts min(chunks, 8) workgroups per image from the handle's own hw; mzlc_create refuses hw > 240 (8 chunks), so its chunk loop cannot
    be reached through a board handle: a 19 x 19 net is refused by name."""
    from muzero_amd.hip_learner import LearnerError

    with pytest.raises(LearnerError, match='boards up to 240 points'):
        _learner(('board19', 'board', (5, 19, 19), 362, 1, 8, 1, 1, 33))


# ------------------------------------------------------------------------------------------ normalize
@pytest.mark.parametrize('C', ac.ENTRY_C)
def test_normalize_bits(atari, boards, C):
    for hw in sorted(ac.ENTRY_HW):
        for B, cls in ((1, 'pow2'), (3, 'float'), (3, 'flat'), (1, 'ties')):
            x = ac.entry_case(cls, B, C, hw)['x']
            s, name = atari.debug_atari_stage('normalize', x=x.reshape((B, C) + ac.ENTRY_HW[hw]))
            assert np.array_equal(s.reshape(B, C, hw).view(np.uint32), ac.normalize_ref(x).view(np.uint32)), (name, cls, B, hw)
    x = ac.entry_case('float', 3, C, 225)['x']
    s, name = boards['board15'].debug_atari_stage('normalize', x=x.reshape(3, C, 15, 15))  # a board handle, a ragged last chunk
    assert np.array_equal(s.reshape(3, C, 225).view(np.uint32), ac.normalize_ref(x).view(np.uint32)), name


# ------------------------------------------------------------------------------------------ gather
# 24 x 24 with B = 1, 2, 3: 4, 8, 12 tiles -- the XCD remap not taken, taken, not taken; 48 x 48: 12 wide tiles (4 x 3) or 16 narrow ones (4 x 4)
GATHER_PLANES = ((24, 24, 1, 'atari'), (24, 24, 2, 'atari'), (24, 24, 3, 'atari'), (48, 48, 1, 'atari'), (48, 48, 1, 'narrow'))


@pytest.mark.parametrize('H,W,B,which', GATHER_PLANES, ids=str)
def test_gather_equals_the_numpy_gather(atari, narrow, H, W, B, which):
    hl = atari if which == 'atari' else narrow
    tw = ac.tile_w(W, which == 'atari')
    for C in (5, 16):  # 5 x 14 x 14 = 980 elements: the tail of the one 1024-element chunk; 16: several chunks and a tail
        for stride, origins in ((1, ((0, 0),)), (2, PARITIES)):
            src0, src1, coef = ac.gather_case(B, C, H, W, stride)
            for origin in origins:
                for mode in ('ident', 'bnrelu', 'bnbwd'):
                    for inner_only in (False, True):
                        kw = {} if mode == 'ident' else dict(coef=coef)
                        if mode == 'bnbwd':
                            kw['src1'] = src1
                        t, name = hl.debug_atari_stage('gather', src0=src0, mode=mode, stride=stride, origin=origin, inner_only=inner_only, **kw)
                        ref = ac.gather_ref(src0, src1, coef, mode, stride, origin, inner_only, tw)
                        _same(t, ref, name)
                        ntiles = B * (H // 12) * (W // tw)
                        assert f'tile=12x{tw} tiles={ntiles} ' in name and f'remap={1 if ntiles % 8 == 0 else 0} ' in name, name


# ------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize('H,W,B,which', ((24, 24, 2, 'atari'), (24, 48, 1, 'atari'), (24, 48, 1, 'narrow'), (12, 12, 3, 'atari')), ids=str)
def test_scatter_equals_the_numpy_scatter(atari, narrow, H, W, B, which):
    hl = atari if which == 'atari' else narrow
    tw = ac.tile_w(W, which == 'atari')
    for C in (5, 24):
        for src_inner in (False, True):
            for stride, origins in ((1, ((0, 0),)), (2, PARITIES)):
                tiles, skip = ac.scatter_case(B, C, H, W, tw, src_inner, stride)
                for origin in origins:
                    for sk in (None, skip):
                        out, name = hl.debug_atari_stage('scatter', tiles=tiles, H=H, W=W, stride=stride, origin=origin, skip=sk, src_inner=src_inner)
                        ref, _ = ac.scatter_ref(tiles, B, H, W, tw, stride, origin, sk, src_inner)
                        assert np.array_equal(np.isnan(out), np.isnan(ref)), name  # NaN exactly where this parity does not write
                        assert np.array_equal(out[~np.isnan(ref)], ref[~np.isnan(ref)]), name


@pytest.mark.parametrize('C', (5, 24, 72, 136))
def test_scatter_statistics_are_the_pivoted_chunk_sums(atari, C):
    B, H, W = 2, 12, 12  # 144 positions: the last 32-position chunk holds 16
    for src_inner in (False, True):
        tiles, skip = ac.scatter_case(B, C, H, W, 12, src_inner, 1)
        for sk in (None, skip):
            out, name, part = atari.debug_atari_stage('scatter', tiles=tiles, H=H, W=W, skip=sk, src_inner=src_inner, want_stats=True)
            ref, v = ac.scatter_ref(tiles, B, H, W, 12, 1, (0, 0), sk, src_inner)
            _same(out, ref, name)
            want = ac.scatter_stats(v)
            assert part.shape == (B * 5, (C + 15) // 16 * 16, 4)
            assert np.array_equal(part[:, :C].astype(np.float64), want), name


# ------------------------------------------------------------------------------------------ refusals
def test_bad_calls_are_refused_by_name(atari, boards):
    from muzero_amd.hip_learner import LearnerError

    f = np.float32
    bad = [
        (atari, 'gather', dict(src0=np.ones((1, 4, 20, 24), f)), r'H: the tiled plane\'s height must be a multiple of 12'),
        (atari, 'scatter', dict(tiles=np.ones((1, 4, 14, 14), f), H=12, W=12, stride=2, origin=(2, 0)), r'origin \(py, px\)'),
        (atari, 's2_fwd', dict(weight=np.ones((16, 4, 3, 3), f), x=np.ones((1, 4, 47, 48), f)), 'x: odd source sizes'),
        (atari, 'pool_fwd', dict(x=np.ones((1, 4, 11, 12), f)), 'H, W: odd source sizes'),
        (atari, 'pool_bwd', dict(g=np.ones((1, 4, 49, 6), f)), r'H, W: must be in \[1, 96\]'),
        (atari, 'normalize', dict(x=np.ones((1, 1025, 6, 6), f)), r'C \(cin\): must be in \[1, 1024\]'),
        (atari, 'entry', dict(x=np.ones((1, 8, 6, 6), f), gs=np.ones((1, 8, 6, 6), f)), r'in3 \(partner\): null argument'),
        (atari, 'entry', dict(x=np.ones((1, 8, 5, 5), f), partner=np.ones((1, 8, 5, 5), f), launcher='tower'), r'hw \(H, W\): launcher tower'),
        (boards['board3'], 'entry', dict(x=np.ones((1, 16, 6, 6), f), partner=np.ones((1, 16, 6, 6), f), launcher='tower'), r'hw \(H, W\): launcher tower'),
        (boards['board3'], 'gather', dict(src0=np.ones((1, 4, 24, 24), f)), 'op: s2_fwd, s2_dgrad, gather and scatter need an Atari handle'),
        (atari, 'gather', dict(src0=np.ones((1, 4, 24, 24), f), mode='bnrelu'), 'coef: null argument'),
        (atari, 's2_fwd', dict(weight=np.ones((16, 4, 3, 3), f), x=np.ones((1, 4, 48, 40), f)), 'W: the tiled plane\'s width must divide into tiles'),
    ]
    for hl, op, kw, msg in bad:
        with pytest.raises(LearnerError, match='mzl_debug_atari_stage: .*' + msg) as e:
            hl.debug_atari_stage(op, **kw)
        if op != 's2_fwd' or 'odd' not in msg:  # (the odd source of s2_fwd is caught by the wrapper, which derives H and W from it)
            assert str(e.value).endswith(f'(status {MZL_E_INVALID})'), str(e.value)
    # the handle is as before: an ordinary call still runs
    x, g = ac.pool_case((6, 6))
    assert np.array_equal(atari.debug_atari_stage('pool_fwd', x=x)[0], ac.pool_fwd_ref(x))
