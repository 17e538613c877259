"""One conv layer at a time on the GPU (mz_debug_conv3x3: the planner's own packers, geometry choosers and launcher), both precisions.

a. Against a float64 conv on seeded random data: the relative rms error over the whole output, per output channel and per pixel is at
   most TWICE that of a plain float32 chain (tests/conv_layer_cases.py: chain32) on the same data, computed on the CPU in the same run.
   Any float32 summation order is statistically of the chain's size; the split-bf16 path with any one of its six terms missing is 4.5 to
   18 times the chain (tests/test_conv_layer_host.py), so the bar is above every honest order and below every such defect.  Then the
   same launch with residual + ReLU equals max(0, pre-activation + residual) in float32, and a launch through per-image pointers (the
   search's node-store gather) equals the dense one row by row.
b. bf16x3 only, exactly: integer data whose every partial sum, term by term and in any order, is an exact float32.  The output must EQUAL
   the int64 conv.  Three classes need (hh, hm, hl), (hh, mh, lh) and (hh, hm, mh, mm); their weight draws cover every (input channel,
   tap) of every output channel, so a wrong lane, octet, tap offset or term plane anywhere in the LDS slab or the w3 stream meets a value
   that needs it.
c. The hook leaves the handle alone: a search before and after a hook call gives the same bits.

Batches: the smallest that give every per-channel and per-pixel slice at least 256 values."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import conv_layer_cases as cc
from helpers import build_conv, build_mlp, conv_case, mlp_case

pytestmark = pytest.mark.gpu

BAR = 2.0  # E(kernel) <= BAR * E(chain32), every statistic
MIN_SLICE = 256

# id: (h, w, cin_real, cin, num_actions, cout, batch at least, words of the split build's name)
CASES = {
    'g3_9to8': (3, 3, 9, 9, 0, 8, 64, ('shape-generic',)),            # one tile, 9 of 64 pixel slots, channels padded 9 -> 32, cout < 16
    'g9_40to48': (9, 9, 40, 40, 0, 48, 4, ('shape-generic',)),        # four ragged tiles, two channel blocks (the second ragged), cout % 32 != 0
    'g10x17_32to16': (10, 17, 32, 32, 0, 16, 2, ('shape-generic',)),  # 2 x 3 tiles, non-square
    'g17_32to16': (17, 17, 32, 32, 0, 16, 2, ('shape-generic',)),     # three tiles per side
    'g7_48a50to48': (7, 7, 48, 98, 50, 48, 6, ('shape-generic',)),    # action planes generated while staging (the p48 net's dynamics conv)
    'w15_64to64': (15, 15, 64, 64, 0, 64, 2, ('SIDE=15', 'NCT=1')),
    'w19_32to24': (19, 19, 32, 32, 0, 24, 2, ('SIDE=19', 'NCT=1')),   # cout with a partial tile
    'w15_128to80': (15, 15, 128, 128, 0, 80, 2, ('SIDE=15', 'NCT=2')),   # five channel tiles: clamped duplicate tiles
    'w15_32to136': (15, 15, 32, 32, 0, 136, 2, ('SIDE=15', 'NCT=2')),    # the second blockIdx.z has one live tile
    'w19_128to128': (19, 19, 128, 128, 0, 128, 2, ('SIDE=19', 'NCT=2')),  # K = 1152: the thinnest margin
}
ROWS_CASES = ('g9_40to48', 'w15_128to80')
PRECISIONS = ('f32', 'bf16x3')


def _batch(case):
    h, w, _, _, _, cout, b0, _ = CASES[case]
    return max(b0, -(-MIN_SLICE // cout), -(-MIN_SLICE // (h * w)))


@functools.lru_cache(maxsize=None)
def _reference(case):
    """Data, float64 reference and the chain's three statistics of a case: computed once, shared by both precisions, never written to."""
    h, w, cr, cin, A, cout, _, _ = CASES[case]
    B = _batch(case)
    d = cc.random_layer(sorted(CASES).index(case) + 1000, B, cr, cin, cout, h, w, num_actions=A)
    kw = dict(bias=d['bias'], action=d['action'], num_actions=A, cin=cin)
    ref = cc.conv64(d['x'], d['w'], **kw)
    c32 = cc.chain32(d['x'], d['w'], **kw)
    assert min(B * h * w, B * cout) >= MIN_SLICE
    e_chain = {s: cc.rel_rms(c32, ref, ax) for s, ax in cc.SLICES.items()}
    for a in list(d.values()) + [ref]:
        if a is not None:
            a.setflags(write=False)
    return d, ref, e_chain


_HANDLES = {}


@pytest.fixture(scope='module')
def handle():
    """precision -> a board-net planner whose conv_precision it is (the hook takes its stream and its precision, nothing else)."""
    from muzero_amd import planner as pl

    def get(precision):
        if precision not in _HANDLES:
            net = build_conv(conv_case('board3'))
            p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=4, conv_precision=precision), 0)
            p.load_state_dict(net.state_dict())
            _HANDLES[precision] = p
        return _HANDLES[precision]

    yield get
    for p in _HANDLES.values():
        p.close()
    _HANDLES.clear()


def _launch(p, case, **kw):
    _, _, _, cin, A, _, _, _ = CASES[case]
    d, _, _ = _reference(case)
    return p.debug_conv3x3(d['x'], d['w'], d['bias'], action=d['action'], num_actions=A, cin=cin, **kw)


def measure(p, case):
    """(pre-activation output, build name, {statistic: (E kernel, E chain32)})."""
    _, ref, e_chain = _reference(case)
    out, name = _launch(p, case)
    return out, name, {s: (cc.rel_rms(out, ref, ax), e_chain[s]) for s, ax in cc.SLICES.items()}


# ------------------------------------------------------------------------------------------ a. float64 accuracy
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(CASES))
def test_layer_matches_float64_within_twice_a_float32_chain(handle, case, precision):
    p = handle(precision)
    out, name, stats = measure(p, case)
    print(f'{case} {precision}: {name}')
    for s, (e, ec) in stats.items():
        r = np.asarray(e / ec)
        print(f'  {s}: E kernel {np.max(e):.3g} (max), E chain32 {np.max(ec):.3g} (max), ratio max {r.max():.3f} median {np.median(r):.3f} over {r.size} slices')
    assert name
    if precision == 'bf16x3':
        for word in CASES[case][7]:
            assert word in name, f'{case}: expected a {word} build, ran {name}'
    for s, (e, ec) in stats.items():
        assert np.all(e <= BAR * ec), f'{case} {precision} {s}: E = {np.max(e / ec):.3f} x chain32 (bar {BAR})'
    # the epilogue is plain float32: + residual, ReLU on the kernel's own pre-activation
    d, _, _ = _reference(case)
    out2, name2 = _launch(p, case, residual=d['residual'], relu=True)
    assert name2 == name
    np.testing.assert_array_equal(out2, np.maximum(out + d['residual'], np.float32(0)))
    assert 0.2 < (out2 == 0).mean() < 0.8  # the ReLU clamps and passes
    if case in ROWS_CASES:  # node-store gather: a permutation of the rows with a repeat
        B = out.shape[0]
        rows = np.random.RandomState(B).permutation(B).astype(np.int32)
        rows[-1] = rows[0]
        out3, name3 = _launch(p, case, rows=rows)
        assert name3 == name
        np.testing.assert_array_equal(out3, out[rows])


# ------------------------------------------------------------------------------------------ b. exact integer checks
# id: (h, w, cin_real, cin, num_actions, cout, words of the build's name)
INT_SHAPES = {
    'g9_40to48': (9, 9, 40, 40, 0, 48, ('shape-generic',)),          # generic, two channel blocks
    'w15_64to80': (15, 15, 64, 64, 0, 80, ('SIDE=15', 'NCT=2')),     # whole image, duplicate tiles
    'g9_40a82to48': (9, 9, 40, 122, 82, 48, ('shape-generic',)),     # action planes: 1 = h, m = l = 0
}
INT_RUNS = [(c, s) for c in cc.INT_CLASSES for s in ('g9_40to48', 'w15_64to80')] + [('W', 'g9_40a82to48')]


@pytest.mark.parametrize('cls,shape', INT_RUNS)
def test_integer_layer_is_exact(handle, cls, shape):
    h, w, cr, cin, A, cout, words = INT_SHAPES[shape]
    B = 2
    p = handle('bf16x3')
    seed = 7 * sorted(INT_SHAPES).index(shape) + sorted(cc.INT_CLASSES).index(cls)
    x = cc.int_input(cls, 200 + seed, B, cr, h, w)
    action = np.array([3, A - 1], np.int32) if A else None
    xf = cc.full_input(x, action, A, cin)
    draws = cc.int_draws(cls, 300 + seed, cin, cout)
    assert cc.covered(draws).all()
    worst = 0
    for i, (wt, bias) in enumerate(draws):
        plain, terms = cc.int_bounds(xf, wt, bias)
        assert plain < 2 ** 23 and terms < 2 ** 24, f'draw {i}: not exact in float32'
        worst = max(worst, plain)
        out, name = p.debug_conv3x3(x, wt, bias, action=action, num_actions=A, cin=cin)
        for word in words:
            assert word in name
        ref = cc.int_reference(xf, wt, bias).astype(np.float32)
        bad = np.argwhere(out != ref)
        assert len(bad) == 0, (f'class {cls} {shape} draw {i} (input channels {cc._live(wt).tolist()}): {len(bad)} outputs differ, first at (image, channel, y, x) = '
                               f'{bad[0].tolist()}: {out[tuple(bad[0])]} != {ref[tuple(bad[0])]}')
    print(f'class {cls} {shape}: {len(draws)} launches, max sum |x||w| + |bias| = {worst:.4g}')


# ------------------------------------------------------------------------------------------ c. the hook and its handle
def test_hook_leaves_the_handle_alone():
    from muzero_amd import planner as pl

    case = conv_case('board3')
    net = build_conv(case)
    B, S, A = 4, 8, case[3]
    kw = dict(num_simulations=S, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, conv_precision='bf16x3', **kw), 0)
    p.load_state_dict(net.state_dict())
    rs = np.random.RandomState(5)
    obs = rs.uniform(0, 1, size=(B,) + tuple(case[2])).astype(np.float32)
    rng = dict(noise=rs.dirichlet(np.full(A, 0.25), size=B), u_tie=rs.rand(B, 4 * S + 8), u_final=rs.rand(B))
    search = lambda: p.search(obs, np.ones((B, A), bool), 1, 2, 1.0, False, **rng)  # noqa: E731
    packed = p.read_packed()
    before = search()
    d = cc.random_layer(1, 3, 16, 16, 16, 3, 3)
    out, name = p.debug_conv3x3(d['x'], d['w'], d['bias'], residual=d['residual'], relu=True)
    assert 'shape-generic' in name and np.isfinite(out).all()
    after = search()
    for k in ('visits', 'pi', 'action', 'root_value'):
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    assert p.read_packed() == packed
    p.close()


def test_hook_refusals(handle):
    from muzero_amd import planner as pl

    p = handle('bf16x3')
    ok = cc.random_layer(2, 1, 4, 4, 4, 3, 3)
    p.debug_conv3x3(ok['x'], ok['w'])
    for x_shape, w_shape, kw in (((1, 4, 2, 3), (4, 4, 3, 3), {}), ((1, 4, 3, 20), (4, 4, 3, 3), {}), ((0, 4, 3, 3), (4, 4, 3, 3), {}),
                                 ((1, 4, 3, 3), (4, 3, 3, 3), dict(cin=3)), ((1, 4, 3, 3), (4, 6, 3, 3), dict(cin=6))):
        with pytest.raises(pl.PlannerError, match='mz_debug_conv3x3'):
            p.debug_conv3x3(np.zeros(x_shape, np.float32), np.zeros(w_shape, np.float32), **kw)
    net = build_mlp(mlp_case('tiny'))
    q = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=2), 0)
    with pytest.raises(pl.PlannerError, match='MZ_NET_MLP'):
        q.debug_conv3x3(ok['x'], ok['w'])
    q.close()


if __name__ == '__main__':  # python tests/test_gpu_conv_layer.py <out.json>: the whole-output ratios of every case, as the tests measure them
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from muzero_amd import planner as pl

    board3 = build_conv(conv_case('board3'))
    result = {'statistic': 'rms(out - conv64) / rms(conv64) over the whole output; ratio = kernel / chain32', 'bar': BAR, 'cases': {}}
    for prec in PRECISIONS:
        planner = pl.Planner(pl.make_mz_config(board3.planner_spec(), None, num_envs=4, conv_precision=prec), 0)
        planner.load_state_dict(board3.state_dict())
        for cid in CASES:
            _, build, st = measure(planner, cid)
            e_k, e_c = (float(v) for v in st['whole'])
            worst_slice = max(float(np.max(st[s][0] / st[s][1])) for s in ('channel', 'pixel'))
            entry = result['cases'].setdefault(cid, {'shape': dict(zip(('h', 'w', 'cin_real', 'cin', 'num_actions', 'cout'), CASES[cid][:6]), batch=_batch(cid)),
                                                     'chain32': float('%.4g' % e_c)})
            entry[prec] = {'kernel': float('%.4g' % e_k), 'ratio': round(e_k / e_c, 4), 'worst_slice_ratio': round(worst_slice, 4), 'build': build}
        planner.close()
    with open(sys.argv[1], 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result, indent=1))
