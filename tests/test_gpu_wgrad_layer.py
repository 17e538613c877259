"""The conv learner's WEIGHT gradient, one launch at a time (HipLearner.debug_wgrad -> mzl_debug_wgrad: the update's own op builders
Sched::wgrad_ops / wgrad_ops_steps / AtariRun::wgrad_tile_ops, make_geom and launch_ops; k_lc_wgrad, k_lc_wgrad_act, k_lc_wgrad_act_reduce and
k_lc_wreduce of muzero_amd/csrc/mz_learn_conv.h).

1. Integer data whose every partial sum is an exact float32 in any order (tests/wgrad_layer_cases.py classes Locator, Dense, Wide;
   tests/test_wgrad_layer_host.py checks the bounds, the Locator's coverage and that every plausible mistake changes the reference): the output
   EQUALS the int64 reference -- at the update's own choices, at every SG the budget allows (side by side and stacked), forced images per chunk,
   both action routes, accumulate, pairs (XCD remap on and off), the K-steps launch, the staging transforms, and the Atari tile builds (ring_rows
   0 .. 3, the four tap sets).  The hook's name says what ran; every case asserts it ran what it is there for.
2. Seeded random data against float64: relative rms error over the whole tensor, per output channel, per input channel and per tap at most
   BAR = 2 x that of a plain sequential float32 chain (bar and slice size of tests/test_gpu_conv_layer.py).
3. Refusals.  4. The weight gradient is float32 at both conv_precision settings: equal bytes, the same kernel."""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import conv_layer_cases as cc
import wgrad_layer_cases as wc
from helpers import build_conv, build_mlp, conv_case, mlp_case
from test_gpu_conv_layer import BAR, MIN_SLICE
from test_wgrad_layer_host import preload, shape_cases, steps_data, tile_cases, transform_cases

pytestmark = pytest.mark.gpu

_HANDLES = {}


def _make(kind):
    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    if kind == 'atari':
        return HipLearner(build_conv(conv_case('atari_s')).to(dev), dev, 5, 2, lr=1e-3)
    return HipLearner(build_conv(conv_case('board3')).to(dev), dev, 5, 4, lr=1e-3, conv_precision=kind)


@pytest.fixture(scope='module')
def handle():
    """'f32' | 'bf16x3' -> a small board-net learner of that conv_precision; 'atari' -> the suite's small Atari learner (the hook takes the
    handle's switches, CU count and -- mode ring -- tile geometries, nothing else)."""
    def get(kind='f32'):
        if kind not in _HANDLES:
            _HANDLES[kind] = _make(kind)
        return _HANDLES[kind]

    yield get
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def ran(name):
    """The hook's name as a dict: 'key=value' fields, 'layout' (single | cols | rows), 'build' (the kernel instantiation), 'precision'."""
    d = dict(re.findall(r'(\w+)=(\S+)', name))
    parts = name.split()
    d['precision'], d['build'] = parts[0], parts[1]
    d['layout'] = next(p for p in parts if p in ('single', 'cols', 'rows'))
    return d


def check_ran(name, what, **want):
    got = ran(name)
    for k, v in want.items():
        assert str(got.get(k)) == str(v), f'{what}: expected {k}={v}, the hook ran "{name}"'


def assert_equal(out, ref, what, name, locate=None):
    msg = wc.first_difference(out, np.asarray(ref, np.float32))
    if msg and locate is not None:
        i = tuple(np.argwhere(out != np.asarray(ref, np.float32))[0])
        msg += f' -- the kernel\'s value is {wc.locate(out[i], *locate)}, the reference\'s {wc.locate(np.asarray(ref)[i], *locate)}'
    assert msg is None, f'{what} ({name}): {msg}'


@functools.lru_cache(maxsize=None)
def _ref(key, cls, i, sg, ipw):
    """The int64 reference of one draw: computed once, shared by every run of the shape, never written to."""
    _, _, dz, x, kw = [c for c in shape_cases(key, sg, ipw) if c[0] == cls and c[1] == i][0]
    ref = wc.wgrad64(dz, x, dtype=np.int64, **kw)
    ref.setflags(write=False)
    return ref


def _int_cases(key, sg, ipw):
    """(class, draw, dz, x, kw, reference); the Locator's draws follow the run's (sg, ipw), the other classes' do not."""
    return [(cls, i, dz, x, kw, _ref(key, cls, i, *((sg, ipw) if cls == 'locator' else (1, 1)))) for cls, i, dz, x, kw in shape_cases(key, sg, ipw)]


# ------------------------------------------------------------------------------------------ 1a. plain launches, the update's choices and forced ones
@pytest.mark.parametrize('rid', list(wc.PLAIN_RUNS))
def test_integer_weight_gradient_is_exact(handle, rid):
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    e = run['expect']
    hl = handle()
    n = 0
    for cls, i, dz, x, kw, ref in _int_cases(run['shape'], e['sg'], e['ipw']):
        out, name = hl.debug_wgrad(dz, x, **kw, **run['over'])
        what = f'{rid} class {cls} draw {i}'
        check_ran(name, what, mode='plain', SG=e['sg'], layout=e['layout'], ipw=e['ipw'], act=e['act'], precision='f32',
                  build='k_lc_wgrad<ACT=1,RING=0>' if e['act'] == 'kernel' else 'k_lc_wgrad<ACT=0,RING=0>', **({} if e['remap'] is None else dict(remap=e['remap'])))
        assert_equal(out, ref, what, name, locate=(B, cr, board, board) if cls == 'locator' and not A else None)
        n += 1
    print(f'{rid}: {n} launches EQUAL, {name}')


@pytest.mark.parametrize('key,layout,sg', [(k, lay, sg) for k, v in wc.SG_REFUSED.items() for lay, sg in v])
def test_an_sg_over_the_lane_or_lds_budget_is_refused_not_launched(handle, key, layout, sg):
    from muzero_amd.hip_learner import LearnerError

    _, _, dz, x, kw = shape_cases(key)[0]
    with pytest.raises(LearnerError, match='mzl_debug_wgrad: SG override'):
        handle().debug_wgrad(dz, x, sg=sg, layout=layout, **kw)


# ------------------------------------------------------------------------------------------ 1b. accumulate
@pytest.mark.parametrize('rid', wc.ACCUMULATE_RUNS)
def test_accumulate_adds_to_a_nonzero_preload(handle, rid):
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    pre = preload(cout, cin)
    for cls, i, dz, x, kw, ref in _int_cases(run['shape'], run['expect']['sg'], run['expect']['ipw']):
        out, name = handle().debug_wgrad(dz, x, preload=pre, accumulate=True, **kw, **run['over'])
        check_ran(name, rid, act=run['expect']['act'], SG=run['expect']['sg'], ipw=run['expect']['ipw'])
        assert_equal(out, ref + pre.astype(np.int64), f'{rid} accumulate class {cls} draw {i}', name)
        out, name = handle().debug_wgrad(dz, x, preload=pre, accumulate=False, **kw, **run['over'])  # and without the flag the preload is overwritten
        assert_equal(out, ref, f'{rid} overwrite class {cls} draw {i}', name)
    print(f'{rid}: accumulate EQUAL, {name}')


# ------------------------------------------------------------------------------------------ 1c. the staging transforms
@pytest.mark.parametrize('rid', wc.TRANSFORM_RUNS)
def test_staging_transforms_are_exact_on_the_wide_class(handle, rid):
    run = wc.PLAIN_RUNS[rid]
    for cls, i, dz, x, kw in transform_cases(rid):
        ref = wc.wgrad64(dz, x, dtype=np.int64, **kw)
        out, name = handle().debug_wgrad(dz, x, **kw, **run['over'])
        check_ran(name, rid, SG=run['expect']['sg'], ipw=run['expect']['ipw'])
        assert_equal(out, ref, f'{rid} {"dcoef + xcoef (IN_BNRELU)" if "xcoef" in kw else "dcoef, identity x"}', name)
    print(f'{rid}: transforms EQUAL, {name}')


# ------------------------------------------------------------------------------------------ 1d. two layers in one launch
@pytest.mark.parametrize('pid', list(wc.PAIR_RUNS))
def test_paired_launch_is_exact_for_both_layers(handle, pid):
    first, second, over, (sg, ipw, remap) = wc.PAIR_RUNS[pid]
    a, b = _int_cases(first, sg, ipw), _int_cases(second, sg, ipw)
    assert (wc.SHAPES[first][1:5] != wc.SHAPES[second][1:5]) == pid.startswith('different')
    for k in range(max(len(a), len(b))):
        (ca, ia, dza, xa, _, refa), (cb, ib, dzb, xb, _, refb) = a[k % len(a)], b[(k + 1) % len(b)]  # (another class in the other layer)
        (outa, outb), name = handle().debug_wgrad(dza, xa, mode='pair', second=dict(dz=dzb, x=xb), **over)
        check_ran(name, pid, mode='pair', SG=sg, ipw=ipw, remap=remap)
        assert_equal(outa, refa, f'{pid} first layer {first} class {ca} draw {ia}', name)
        assert_equal(outb, refb, f'{pid} second layer {second} class {cb} draw {ib}', name)
    print(f'{pid}: pair EQUAL, {name}')


# ------------------------------------------------------------------------------------------ 1e. the K-steps launch
@pytest.mark.parametrize('sid', list(wc.STEP_RUNS))
def test_steps_launch_is_exact(handle, sid):
    key, nsrc, over, (sg, ipw, cps) = wc.STEP_RUNS[sid]
    for cls, i, dz, x in steps_data(key, nsrc):
        ref = wc.wgrad64(dz.reshape((-1,) + dz.shape[2:]), x.reshape((-1,) + x.shape[2:]), dtype=np.int64)
        out, name = handle().debug_wgrad(dz, x, mode='steps', **over)
        check_ran(name, sid, mode='steps', SG=sg, ipw=ipw, cps=cps, nsrc=nsrc, chunks=nsrc * cps)
        assert_equal(out, ref, f'{sid} class {cls} draw {i}', name)
    print(f'{sid}: steps EQUAL, {name}')


def test_steps_launch_applies_each_sources_own_coefficients(handle):
    key, nsrc = 'b9_8to8_n5', 2
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    d = [wc.wide_transform_draw(900 + s, B, cr, cout, board, board) for s in range(nsrc)]
    st = {k: np.stack([e[k] for e in d]) for k in d[0]}
    ref = sum(wc.wgrad64(e['dz'], e['x'], dtype=np.int64, y=e['y'], dcoef=e['dcoef'], xcoef=e['xcoef']) for e in d)
    assert sum(wc.int_bound(e['dz'], e['x'], y=e['y'], dcoef=e['dcoef'], xcoef=e['xcoef'])[0] for e in d) < 2 ** 24
    out, name = handle().debug_wgrad(st['dz'], st['x'], mode='steps', y=st['y'], dcoef=st['dcoef'], xcoef=st['xcoef'])
    check_ran(name, 'steps with transforms', mode='steps', nsrc=nsrc)
    assert_equal(out, ref, 'steps with per-source dcoef and xcoef', name)


# ------------------------------------------------------------------------------------------ 1f. the Atari tile builds
@pytest.mark.parametrize('key,ring_rows,ipw', wc.RING_RUNS)
def test_ring_builds_are_exact(handle, key, ring_rows, ipw):
    h, w, cr, cout, B = wc.ATARI_TILES[key]
    hl = handle('atari')
    for cls, i, dz, x, kw in tile_cases(key):
        ref = wc.wgrad64(dz, x, dtype=np.int64, ring=True)
        out, name = hl.debug_wgrad(dz, x, mode='ring', ring_rows=ring_rows, ipw=ipw)
        check_ran(name, key, mode='ring', ring_rows=ring_rows, SG=1, taps='0x1ff', nsteps=wc.RING_NSTEPS[h, w, ring_rows], build='k_lc_wgrad<ACT=0,RING=1>',
                  ipw=ipw or 1, chunks=-(-B // (ipw or 1)))
        assert_equal(out, ref, f'{key} ring_rows {ring_rows} ipw {ipw} class {cls} draw {i}', name, locate=(B, cr, h, w) if cls == 'locator' else None)
    print(f'{key} ring_rows {ring_rows} ipw {ipw}: EQUAL, {name}')


@pytest.mark.parametrize('mask', wc.TAPMASKS, ids=[f'{m:#05x}' for m in wc.TAPMASKS])
@pytest.mark.parametrize('key,ring_rows', [('t14x18_4to128_n2', 2), ('t14x14_128to128_n3', 3), ('t14x14_4to16_n3', 1), ('t14x18_4to128_n2', 0)])
def test_tap_sets_write_their_taps_and_leave_the_others(handle, key, ring_rows, mask):
    """A parity plane of a stride-2 conv: only the mask's accumulators exist; k_lc_wreduce's tap map writes them to the plane's weight taps and
    touches no other tap of the output -- those still hold the preload."""
    h, w, cr, cout, B = wc.ATARI_TILES[key]
    pre = preload(cout, cr)
    for cls, i, dz, x, kw in tile_cases(key):
        ref = wc.apply_tapmask(wc.wgrad64(dz, x, dtype=np.int64, ring=True), mask, pre)
        out, name = handle('atari').debug_wgrad(dz, x, mode='ring', ring_rows=ring_rows, tapmask=mask, preload=pre)
        check_ran(name, key, mode='ring', ring_rows=ring_rows, taps=f'{mask:#05x}', build='k_lc_wgrad<ACT=0,RING=1,TAPS>')
        assert_equal(out, ref, f'{key} ring_rows {ring_rows} taps {mask:#05x} class {cls} draw {i}', name)
    print(f'{key} ring_rows {ring_rows} taps {mask:#05x}: EQUAL, {name}')


# ------------------------------------------------------------------------------------------ 2. random data against float64
# id: (board, cin, cout, batch, ipw override): reductions of B * board^2 = 2 025 | 2 250 terms (the ring case: 12 x 144 = 1 728); every slice has MIN_SLICE values
RANDOM_CASES = {'b9_40to48': (9, 40, 48, 25, 0), 'b9_40to48_ipwB': (9, 40, 48, 25, 25), 'b15_64to80': (15, 64, 80, 10, 0), 'b15_64to80_ipwB': (15, 64, 80, 10, 10)}
RANDOM_RING = ('t14x14_64to48', (14, 14, 64, 48, 12))  # 12 tiles x 144 inner positions


@functools.lru_cache(maxsize=None)
def _random_reference(board_h, board_w, cin, cout, B, ring):
    rs = np.random.RandomState(3000 + board_h * board_w + cin)
    x, dz = cc.random_values(rs, (B, cin, board_h, board_w), (B, cout, board_h, board_w))
    ref = wc.wgrad64(dz, x, ring=ring)
    c32 = wc.chain32(dz, x, ring=ring)
    assert min(cin * 9, cout * 9, cin * cout) >= MIN_SLICE
    e_chain = {s: cc.rel_rms(c32, ref, ax) for s, ax in wc.SLICES.items()}
    for a in (x, dz, ref):
        a.setflags(write=False)
    return dz, x, ref, e_chain


def measure_random(hl, cid):
    """(name, {slice: (E kernel, E chain32)}) of one random case."""
    if cid == RANDOM_RING[0]:
        h, w, cin, cout, B = RANDOM_RING[1]
        dz, x, ref, e_chain = _random_reference(h, w, cin, cout, B, True)
        out, name = hl.debug_wgrad(dz, x, mode='ring')
    else:
        board, cin, cout, B, ipw = RANDOM_CASES[cid]
        dz, x, ref, e_chain = _random_reference(board, board, cin, cout, B, False)
        out, name = hl.debug_wgrad(dz, x, ipw=ipw)
        if ipw:
            check_ran(name, cid, ipw=ipw, chunks=1)
    return name, {s: (cc.rel_rms(out, ref, ax), e_chain[s]) for s, ax in wc.SLICES.items()}


@pytest.mark.parametrize('cid', list(RANDOM_CASES) + [RANDOM_RING[0]])
def test_random_weight_gradient_matches_float64_within_twice_a_float32_chain(handle, cid):
    """Measured on an MI355X (profiles/wgrad_layer/accuracy.json): see README."""
    name, st = measure_random(handle('atari' if cid == RANDOM_RING[0] else 'f32'), cid)
    print(f'{cid}: {name}')
    for s, (e, ec) in st.items():
        r = np.asarray(e / ec)
        print(f'  {s}: E kernel {np.max(e):.3g} (max), E chain32 {np.max(ec):.3g} (max), ratio max {r.max():.3f} median {np.median(r):.3f} over {r.size} slices')
    for s, (e, ec) in st.items():
        assert np.all(e <= BAR * ec), f'{cid} {s}: E = {np.max(e / ec):.3f} x chain32 (bar {BAR}), {name}'


# ------------------------------------------------------------------------------------------ 3. refusals
def test_refusals(handle):
    from muzero_amd import hip_learner as hlm

    dev = torch.device('cuda', 0)
    hl, at = handle(), handle('atari')
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    ok = dict(dz=z(2, 8, 3, 3), x=z(2, 4, 3, 3))
    hl.debug_wgrad(**ok)
    tile = dict(dz=z(1, 8, 14, 14), x=z(1, 4, 14, 14))
    at.debug_wgrad(mode='ring', **tile)
    act = dict(action=np.array([0, 9], np.int32), num_actions=10, cin=14)
    bad = [
        (at, dict(ok), 'board handle'),                                              # board modes on an Atari handle
        (hl, dict(tile, mode='ring'), 'Atari handle'),                               # ring on a board handle
        (hl, dict(dz=z(1, 8, 16, 16), x=z(1, 4, 16, 16)), 'h \\* w'),                 # hw outside what make_geom takes
        (at, dict(dz=z(1, 8, 14, 19), x=z(1, 4, 14, 19), mode='ring'), 'h \\* w'),
        (hl, dict(ok, cin=3), 'cin < cin_real'),
        (hl, dict(ok, **dict(act, action=np.array([0, 10], np.int32))), 'action out of'),
        (hl, dict(ok, **dict(act, action=np.array([-1, 0], np.int32))), 'action out of'),
        (hl, dict(ok, cin=14, num_actions=10), 'needs action'),
        (hl, dict(ok, **dict(act, cin=15), act_route=2), 'sparse action route'),     # 11 planes of 10 actions: the gather is one thread per action
        (hl, dict(ok, sg=22), 'SG override'),
        (hl, dict(ok, ipw=3), 'ipw override'),
        (hl, dict(ok, ring_rows=1), 'mode ring'),
        (hl, dict(ok, tapmask=0x010), 'mode ring'),
        (hl, dict(ok, y=z(2, 8, 3, 3)), 'y and dcoef'),
        (at, dict(tile, mode='ring', sg=2, ring_rows=1), 'SG = 1'),                  # the update checks that too
        (at, dict(tile, mode='ring', tapmask=0x111), 'tap mask'),
        (at, dict(tile, mode='ring', ring_rows=2), 'ring_rows build'),               # 14 x 14: pitch 16, no row steps
        (at, dict(tile, mode='ring', accumulate=True), 'never accumulates'),
    ] + [(at, dict(dz=z(2, 8, *wc.ATARI_TILES[k][:2]), x=z(2, 4, *wc.ATARI_TILES[k][:2]), mode='ring', ring_rows=rr), 'ring_rows build') for k, rr in wc.RING_REFUSED]
    for h, kw, pat in bad:
        with pytest.raises(hlm.LearnerError, match='mzl_debug_wgrad.*' + pat):
            h.debug_wgrad(**kw)
    with pytest.raises(hlm.LearnerError, match="mode 'pair' needs"):
        hl.debug_wgrad(mode='pair', **ok)
    with pytest.raises(hlm.LearnerError, match='mzl_debug_wgrad'):
        hl.debug_wgrad(mode='pair', second=dict(dz=z(2, 8, 3, 3), x=z(2, 4, 3, 3), action=np.array([0, 1], np.int32), cin=14), num_actions=10, **ok)
    # null pointers and a non-conv handle, at the ABI itself
    lib = hlm.load_library()
    name = hlm.C.c_char_p()
    call = hlm.MzlWgradCall()
    call.mode, call.batch, call.h, call.w, call.nsrc = 0, 1, 3, 3, 1
    call.layer[0].cin_real = call.layer[0].cin = call.layer[0].cout = 4
    assert lib.mzl_debug_wgrad(hl._h, hlm.C.byref(call), hlm.C.byref(name)) == -1 and 'mzl_debug_wgrad: null argument' in lib.mzl_last_error().decode()
    assert lib.mzl_debug_wgrad(hl._h, None, hlm.C.byref(name)) == -1 and 'mzl_debug_wgrad: null argument' in lib.mzl_last_error().decode()
    mlp = hlm.HipLearner(build_mlp(mlp_case('tiny')).to(dev), dev, 5, 4, lr=1e-3)
    with pytest.raises(hlm.LearnerError, match='mzl_debug_wgrad: needs a conv-net learner'):
        mlp.debug_wgrad(**ok)
    mlp.close()
    # and a refusal leaves the handle's switches as they were: the same call, the same name
    _, n0 = hl.debug_wgrad(**ok)
    _, n1 = hl.debug_wgrad(**ok)
    assert re.sub(r' us=\S+', '', n0) == re.sub(r' us=\S+', '', n1)


# ------------------------------------------------------------------------------------------ 4. float32 at both precisions
def test_weight_gradient_is_float32_at_both_conv_precisions(handle):
    """README: the weight gradient is NOT split.  Until a split-bf16 weight gradient changes this on purpose, a bf16x3 handle runs the same kernel
    and writes the same bytes."""
    board, cin, cout, B, _ = RANDOM_CASES['b9_40to48']
    dz, x, _, _ = _random_reference(board, board, cin, cout, B, False)
    (o32, n32), (o3, n3) = handle('f32').debug_wgrad(dz, x), handle('bf16x3').debug_wgrad(dz, x)
    assert n32.startswith('f32 k_lc_wgrad<') and n3.startswith('bf16x3 k_lc_wgrad<'), (n32, n3)
    strip = lambda n: re.sub(r' us=\S+', '', n.split(' ', 1)[1])  # noqa: E731
    assert strip(n32) == strip(n3), (n32, n3)
    assert o32.tobytes() == o3.tobytes()


if __name__ == '__main__':  # python tests/test_gpu_wgrad_layer.py <out.json>: the ratios of every random case, as the test measures them
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    result = {'statistic': 'rms(out - wgrad64) / rms(wgrad64); ratio = kernel / chain32 (a sequential float32 sum over images and positions)', 'bar': BAR, 'cases': {}}
    hs = {k: _make(k) for k in ('f32', 'atari')}
    for cid in list(RANDOM_CASES) + [RANDOM_RING[0]]:
        name, st = measure_random(hs['atari' if cid == RANDOM_RING[0] else 'f32'], cid)
        entry = {'ran': re.sub(r' us=\S+', '', name), 'chain32': float('%.4g' % float(st['whole'][1])), 'kernel': float('%.4g' % float(st['whole'][0])),
                 'ratio': round(float(st['whole'][0] / st['whole'][1]), 4)}
        for s in ('cout', 'cin', 'tap'):
            r = np.asarray(st[s][0] / st[s][1])
            entry[f'{s}_slices'] = {'n': int(r.size), 'ratio_min': round(float(r.min()), 4), 'ratio_median': round(float(np.median(r)), 4), 'ratio_max': round(float(r.max()), 4)}
        result['cases'][cid] = entry
    for h in hs.values():
        h.close()
    with open(sys.argv[1], 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result, indent=1))
