"""The conv learner's fused BatchNorm path, one launch at a time (HipLearner.debug_conv_fused -> mzl_debug_conv_fused: the update's own packers, make_geom,
Sched::conv_base / op_conv / op_bnfwd / op_bnbwd / op_apply and launch_ops; k_lc_conv and k_lc_conv_bf16x3 with their staging transforms, write-through,
epilogue and statistics, k_lc_bn_fwd, k_lc_bn_bwd, k_lc_apply), at both conv precisions.

a. Integer data whose every partial sum is an exact float32 in any order (tests/conv_fused_cases.py; tests/test_conv_fused_host.py checks the bounds, the
   properties of every case and that every plausible mistake changes the reference): outputs, write-through and -- class S -- the raw statistics partials
   EQUAL the int64 / float64 reference.  A failure names the case, the draw's input channels, and the (image, channel, y, x) or (group, channel, entry).
b. The finalize kernels from those exact partials and from host-made ones of 1 .. 3001 groups: bars counted from the kernel's roundings, stated beside
   each assertion.
c. Seeded random data against float64 at twice a float32 chain (bar, statistics and slice size of tests/test_gpu_conv_layer.py), and the variance of an
   ill-conditioned output (mean^2 / var about 10^6) at twice the error of a float32 model of the pivoted sums.
d. The write-through of an IN_BNRES conv and k_lc_apply of the same operands: the same bits.
e. Two calls give the same bits, a burst of hook calls leaves the update's gradient bytes alone, refusals."""
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import conv_fused_cases as fc
import conv_layer_cases as cc
from helpers import build_conv, build_mlp, conv_case, mlp_case
from test_conv_fused_host import ILL, forward_refs, rel_rms_over_channels
from test_gpu_conv_layer import BAR, MIN_SLICE

pytestmark = pytest.mark.gpu
PRECISIONS = ('f32', 'bf16x3')
KERNEL = {'f32': 'k_lc_conv', 'bf16x3': 'k_lc_conv_bf16x3'}
POS = ('image', 'channel', 'y', 'x')
PART = ('group', 'channel', 'entry (p, sum, sum of squares, n | sum t, sum t * partner)')
_HANDLES = {}


def _make(kind):
    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    return HipLearner(build_conv(conv_case('board3')).to(dev), dev, 5, 4, lr=1e-3, conv_precision=kind)


@pytest.fixture(scope='module')
def handle():
    """'f32' | 'bf16x3' -> a small board-net learner of that conv_precision (the hook takes its precision, switches and CU count, nothing else)."""
    def get(kind='f32'):
        if kind not in _HANDLES:
            _HANDLES[kind] = _make(kind)
        return _HANDLES[kind]

    yield get
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def ran(name):
    d = dict(re.findall(r'(\w+)=(\S+)', name))
    d['precision'], d['build'] = name.split()[:2]
    return d


def check_ran(name, what, **want):
    got = ran(name)
    for k, v in want.items():
        assert str(got.get(k)) == str(v), f'{what}: expected {k}={v}, the hook ran "{name}"'


def assert_equal(out, ref, names, what, name):
    msg = fc.first_difference(out, np.asarray(ref, np.float32), names)
    assert msg is None, f'{what} ({name}): {msg}'


def check_partials_fwd(part, ref, co, exact, what, name):
    """real channels: (p, n) always, the two sums where the class keeps them exact; padding channels: p = 0 and n = 0."""
    assert part.shape == ref.shape, (what, part.shape, ref.shape)
    ent = (0, 1, 2, 3) if exact else (0, 3)
    assert_equal(part[:, :co][:, :, ent], ref[:, :co][:, :, ent], PART, what + ' partials', name)
    assert_equal(part[:, co:][:, :, (0, 3)], np.zeros_like(part[:, co:][:, :, (0, 3)]), PART, what + ' padding channels (p, n)', name)


# ------------------------------------------------------------------------------------------ a. exact integers
FWD_LIGHT = ('ident', 'bnrelu', 'bnres_mat')   # classes W, X, M: outputs only
DGRAD_LIGHT = ('second_conv', 'first_conv')


def fwd_job(d, wt, stat='fwd', **kw):
    return dict(weight=wt, in0=d['in0'], in1=d['in1'], coef=d['coef'], in_mode=d['mode'], stat=stat, mat_preload=d['mat_preload'], **kw)


def dgrad_job(d, wt, combo, **kw):
    skip, mask, mcoef, partner, stat = fc.DGRAD_COMBOS[combo]
    e = d['epi']
    return dict(weight=fc.dgrad_weight(wt), direction=1, in0=d['in0'], in1=d['in1'], coef=d['coef'], in_mode='bnbwd', skip=e['skip'] if skip else None,
                mask=e['mask'] if mask else None, mcoef=e['mcoef'] if mcoef else None, partner='mask' if partner == 'mask' else (e['partner'] if partner else None), stat=stat, **kw)


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('key', list(fc.GEOMS))
def test_forward_conv_staging_write_through_and_partials_are_exact(handle, key, precision):
    h, w, B, ci, co, no_side, exp = fc.GEOMS[key]
    hl = handle(precision)
    n = 0
    for cls in fc.CLASSES_OF[key]:
        for combo in (fc.FWD_COMBOS if cls == 'S' else FWD_LIGHT):
            d, refs = forward_refs(key, cls, combo)
            for i, wt, ref in refs:
                what = f'{key} {precision} class {cls} {combo} draw {i} (input channels {cc._live(wt).tolist()})'
                r, name = hl.debug_conv_fused(fwd_job(d, wt), no_side=no_side)
                check_ran(name, what, precision=precision, build=KERNEL[precision], mode='IN_' + d['mode'].upper(), stat='ST_FWD', dir='forward', pair=0, **exp)
                assert r['groups'] == exp['groups']
                assert_equal(r['out'], ref, POS, what + ' output', name)
                if d['mat_preload'] is not None:   # the staged operand at every (image, channel, pixel): nothing of the preload is left, nothing else is written
                    assert_equal(r['mat_out'], d['target'], POS, what + ' write-through', name)
                check_partials_fwd(r['part'], fc.partials_fwd(ref, exp['G']), co, cls == 'S', what, name)
                n += 1
    print(f'{key} {precision}: {n} launches EQUAL, {name}')


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('key', list(fc.GEOMS))
def test_data_gradient_staging_epilogue_and_partials_are_exact(handle, key, precision):
    h, w, B, ci, co, no_side, exp = fc.GEOMS[key]
    hl = handle(precision)
    n = 0
    for cls in fc.CLASSES_OF[key]:
        d = fc.dgrad_case(key, cls)
        for combo in (fc.DGRAD_COMBOS if cls == 'S' else DGRAD_LIGHT):
            stat = fc.DGRAD_COMBOS[combo][4]
            for i, (wt, _) in enumerate(d['draws']):
                what = f'{key} {precision} class {cls} dgrad {combo} draw {i} (input channels {cc._live(wt).tolist()})'
                t, part = fc.dgrad_reference(d, wt, combo, exp['G'])
                r, name = hl.debug_conv_fused(dgrad_job(d, wt, combo), no_side=no_side)
                check_ran(name, what, precision=precision, build=KERNEL[precision], mode='IN_BNBWD', stat='ST_BWD' if stat else 'ST_NONE', dir='dgrad', **exp)
                assert_equal(r['out'], t, POS, what + ' output', name)
                if stat and cls == 'S':
                    assert_equal(r['part'][:, :co], part[:, :co], PART, what + ' partials', name)
                n += 1
    print(f'{key} {precision}: {n} launches EQUAL, {name}')


# ------------------------------------------------------------------------------------------ b. the finalize kernels
def check_bn_fwd(r, f, ops, C, what):
    """Bars counted from k_lc_bn_fwd's roundings (f: the float64 reference of the same float32 inputs)."""
    cpad = fc.pad16(C)
    coef, save = r['coef'], r['save']
    assert coef.shape == (3, cpad) and save.shape == (2, cpad)
    assert (coef[:, C:] == 0).all() and (save[:, C:] == 0).all() and (coef[2] == 0).all(), what + ': padding channels / the unused row are zeroed'
    assert (np.abs(save[0, :C] - f['mean']) <= fc.ulp(f['mean'])).all(), what + ' mean: one rounding of a float64 value, 1 ulp'
    assert (np.abs(save[1, :C] - f['invstd']) <= fc.ulp(f['invstd'])).all(), what + ' invstd: one rounding, 1 ulp'
    assert (np.abs(coef[0, :C] - f['a']) <= 2 * fc.ulp(f['a'])).all(), what + ' a = gamma * invstd: the rounding of invstd and of the product, 2 ulp'
    bar_b = 4 * 2.0 ** -24 * np.maximum(np.abs(ops['beta']), np.abs(f['mean'] * f['a']))
    assert (np.abs(coef[1, :C] - f['b']) <= bar_b).all(), what + ' b = beta - mean a: a (2), mean (1), the product and the difference: 4 x 2^-24 x max(|beta|, |mean a|)'
    assert (np.abs(r['running_mean'] - f['running_mean']) <= fc.ulp(f['running_mean'])).all(), what + ' running_mean: one rounding, 1 ulp'
    assert (np.abs(r['running_var'] - f['running_var']) <= fc.ulp(f['running_var'])).all(), what + ' running_var (unbiased): one rounding, 1 ulp'


def check_bn_bwd(r, f, ops, C, accumulate, what):
    cpad = fc.pad16(C)
    coef = r['coef']
    assert coef.shape == (3, cpad) and (coef[:, C:] == 0).all(), what + ': padding channels are zeroed'
    for k, n in enumerate(('c1', 'c2', 'c3')):
        assert (np.abs(coef[k, :C] - f[n]) <= fc.ulp(f[n])).all(), f'{what} {n}: one rounding of a float64 expression of the float32 inputs, 1 ulp'
    if accumulate:   # float32(dgamma before + float32(dgam)): two roundings, one at dgam's size and one at the result's
        assert (np.abs(r['dgamma'] - f['dgamma']) <= fc.ulp(f['dgam']) + fc.ulp(f['dgamma'])).all(), what + ' dgamma (accumulate): 1 ulp of dgam + 1 ulp of the sum'
    else:
        assert (np.abs(r['dgamma'] - f['dgamma']) <= fc.ulp(f['dgamma'])).all(), what + ' dgamma: one rounding, 1 ulp'
    assert np.array_equal(r['dbeta'], f['dbeta'].astype(np.float32)) and np.array_equal(f['dbeta'], np.rint(f['dbeta'])), what + ' dbeta on integer sums: EQUAL'


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('key', ['g3x3', 'g6x6_c24', 'g15_side'])
def test_finalize_behind_the_conv_from_exact_partials(handle, key, precision):
    h, w, B, ci, co, no_side, exp = fc.GEOMS[key]
    hl = handle(precision)
    ops = fc.finalize_operands(31, co)
    d, refs = forward_refs(key, 'S', 'bnres_mat')
    i, wt, ref = refs[-1]
    r, name = hl.debug_conv_fused(fwd_job(d, wt, finalize='fwd', gamma=ops['gamma'], beta=ops['beta'], running_mean=ops['running_mean'], running_var=ops['running_var'],
                                          num_batches=41), no_side=no_side)
    check_ran(name, key, fin='fwd', stat='ST_FWD', **exp)
    part = fc.partials_fwd(ref, exp['G'])
    check_partials_fwd(r['part'], part, co, True, f'{key} {precision} finalize fwd', name)
    f = fc.bn_fwd(part.astype(np.float32), ops['gamma'], ops['beta'], B * h * w, ops['running_mean'], ops['running_var'])
    np.testing.assert_allclose(f['mean'], ref.mean(axis=(0, 2, 3)), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(f['var'], ref.astype(np.float64).var(axis=(0, 2, 3)), rtol=1e-11)
    check_bn_fwd(r, f, ops, co, f'{key} {precision} {name}')
    assert r['num_batches'] == 42   # exactly one more
    # and the data gradient's: second_conv (partner aliased), accumulate on, then off
    dg = fc.dgrad_case(key, 'S')
    wt = dg['draws'][-1][0]
    t, part = fc.dgrad_reference(dg, wt, 'second_conv', exp['G'])
    for acc in (True, False):
        r, name = hl.debug_conv_fused(dgrad_job(dg, wt, 'second_conv', finalize='bwd', gamma=ops['gamma'], save=ops['save'], dgamma=ops['dgamma'], dbeta=ops['dbeta'],
                                                accumulate=acc), no_side=no_side)
        check_ran(name, key, fin='bwd', stat='ST_BWD', **exp)
        assert_equal(r['part'][:, :co], part[:, :co], PART, f'{key} {precision} finalize bwd partials', name)
        f = fc.bn_bwd(part.astype(np.float32), ops['gamma'], ops['save'], B * h * w, ops['dgamma'], ops['dbeta'], accumulate=acc)
        check_bn_bwd(r, f, ops, co, acc, f'{key} {precision} accumulate={acc} {name}')


@pytest.mark.parametrize('groups', fc.FINALIZE_GROUPS)
def test_finalize_only_over_the_group_counts_where_the_loops_change(handle, groups):
    """lc_pivot_sums takes its unrolled loop above 48 groups, lc_group_sums above 112; 16 | 17: one | two groups in slice 0; 3001: the tiled stages' counts."""
    hl = handle()
    C, n = fc.FINALIZE_C, 72
    ops = fc.finalize_operands(5, C)
    pf, pb = fc.finalize_parts(groups, groups, C, 'fwd', n), fc.finalize_parts(groups + 1, groups, C, 'bwd')
    r, name = hl.debug_conv_fused(dict(part=pf, finalize='fwd', gamma=ops['gamma'], beta=ops['beta'], running_mean=ops['running_mean'], running_var=ops['running_var'],
                                       num_batches=7), mode='finalize', count=groups * n)
    check_ran(name, f'{groups} groups', build='k_lc_bn_fwd', groups=groups, C=C, cpad=32)
    check_bn_fwd(r, fc.bn_fwd(pf, ops['gamma'], ops['beta'], groups * n, ops['running_mean'], ops['running_var']), ops, C, name)
    assert r['num_batches'] == 8
    for acc in (False, True):
        r, name = hl.debug_conv_fused(dict(part=pb, finalize='bwd', gamma=ops['gamma'], save=ops['save'], dgamma=ops['dgamma'], dbeta=ops['dbeta'], accumulate=acc),
                                      mode='finalize', count=groups * n)
        check_ran(name, f'{groups} groups', build='k_lc_bn_bwd', groups=groups, C=C, cpad=32, accumulate=int(acc))
        f = fc.bn_bwd(pb, ops['gamma'], ops['save'], groups * n, ops['dgamma'], ops['dbeta'], accumulate=acc)
        assert (f['cancel'] > 2.0 ** -20).all()
        check_bn_bwd(r, f, ops, C, acc, name)


# ------------------------------------------------------------------------------------------ a'. two different layers in one paired launch
@pytest.mark.parametrize('precision', PRECISIONS)
def test_paired_launch_of_two_different_layers(handle, precision):
    ka, kb = 'g6x6', 'g6x6_c24'
    assert fc.GEOMS[ka][:3] == fc.GEOMS[kb][:3] and fc.GEOMS[ka][3:5] != fc.GEOMS[kb][3:5]
    h, w, B, _, _, _, exp = fc.GEOMS[ka]
    hl = handle(precision)
    oa, ob = fc.finalize_operands(41, fc.GEOMS[ka][4]), fc.finalize_operands(42, fc.GEOMS[kb][4])
    (da, ra), (db, rb) = forward_refs(ka, 'S', 'bnres_mat'), forward_refs(kb, 'S', 'bnres_mat')
    fin = lambda o: dict(finalize='fwd', gamma=o['gamma'], beta=o['beta'], running_mean=o['running_mean'], running_var=o['running_var'], num_batches=3)  # noqa: E731
    for k in range(2):
        (ia, wa, refa), (ib, wb, refb) = ra[k % len(ra)], rb[(5 * k + 1) % len(rb)]
        (a, b), name = hl.debug_conv_fused(fwd_job(da, wa, **fin(oa)), mode='pair', second=fwd_job(db, wb, **fin(ob)))
        check_ran(name, 'pair', pair=1, fin='fwd', NPT=exp['NPT'], G=exp['G'], groups=exp['groups'], mode='IN_BNRES')
        for r, d, ref, key, o, i in ((a, da, refa, ka, oa, ia), (b, db, refb, kb, ob, ib)):
            co = fc.GEOMS[key][4]
            what = f'pair {precision} job {key} draw {i}'
            assert_equal(r['out'], ref, POS, what + ' output', name)
            assert_equal(r['mat_out'], d['target'], POS, what + ' write-through', name)
            part = fc.partials_fwd(ref, exp['G'])
            check_partials_fwd(r['part'], part, co, True, what, name)
            check_bn_fwd(r, fc.bn_fwd(part.astype(np.float32), o['gamma'], o['beta'], B * h * w, o['running_mean'], o['running_var']), o, co, what)
            assert r['num_batches'] == 4
    dga, dgb = fc.dgrad_case(ka, 'S'), fc.dgrad_case(kb, 'S')
    wa, wb = dga['draws'][0][0], dgb['draws'][3][0]
    (a, b), name = hl.debug_conv_fused(dgrad_job(dga, wa, 'first_conv'), mode='pair', second=dgrad_job(dgb, wb, 'first_conv'))
    check_ran(name, 'pair dgrad', pair=1, mode='IN_BNBWD', stat='ST_BWD', dir='dgrad')
    for r, d, wt, key in ((a, dga, wa, ka), (b, dgb, wb, kb)):
        t, part = fc.dgrad_reference(d, wt, 'first_conv', exp['G'])
        assert_equal(r['out'], t, POS, f'pair {precision} dgrad job {key} output', name)
        assert_equal(r['part'][:, :fc.GEOMS[key][4]], part[:, :fc.GEOMS[key][4]], PART, f'pair {precision} dgrad job {key} partials', name)


# ------------------------------------------------------------------------------------------ c. random data against float64
# id: (mode, h, w, c_in, c_out, batch): reductions of 360 terms; every per-channel and per-pixel slice has MIN_SLICE values
RANDOM_CASES = {'bnrelu_9x9': ('bnrelu', 9, 9, 40, 48, 6), 'bnres_9x9': ('bnres', 9, 9, 40, 48, 6), 'bnbwd_9x9': ('bnbwd', 9, 9, 40, 48, 6), 'bnres_15x15': ('bnres', 15, 15, 24, 40, 7)}


@functools.lru_cache(maxsize=None)
def _random_data(cid):
    mode, h, w, ci, co, B = RANDOM_CASES[cid]
    rs = np.random.RandomState(4000 + sorted(RANDOM_CASES).index(cid))
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    d = dict(in0=f(rs.randn(B, ci, h, w)), in1=f(rs.uniform(0, 1, (B, ci, h, w)) if mode == 'bnres' else rs.randn(B, ci, h, w)) if mode != 'bnrelu' else None,
             coef=f(np.stack([rs.uniform(0.5, 1.5, ci), rs.randn(ci) * 0.3, rs.randn(ci) * 0.1])), w=f(rs.randn(co, ci, 3, 3) * 0.05), skip=f(rs.randn(B, co, h, w)))
    assert min(B * h * w, B * co) >= MIN_SLICE
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


def measure_random(hl, cid):
    """(name, {slice: (E kernel, E chain32)}, write-through error in float32 ulps or None) of one random case."""
    mode = RANDOM_CASES[cid][0]
    d = _random_data(cid)
    if mode == 'bnbwd':   # the data gradient of a layer c_out -> c_in... run as the effective conv c_in -> c_out, + skip
        r, name = hl.debug_conv_fused(dict(weight=fc.dgrad_weight(d['w']), direction=1, in0=d['in0'], in1=d['in1'], coef=d['coef'], in_mode='bnbwd', skip=d['skip']))
        staged = fc.stage('bnbwd', d['in0'], d['in1'], d['coef'])
        ref = cc.conv_acc(staged, d['w'], np.float64) + d['skip']
        c32 = cc.chain32(staged.astype(np.float32), d['w'], residual=d['skip'])
        mat_ulps = None
    else:   # the reference convolves what the kernel staged (its write-through, held to the integer classes above and to the float32 model here)
        r, name = hl.debug_conv_fused(dict(weight=d['w'], in0=d['in0'], in1=d['in1'], coef=d['coef'], in_mode=mode, stat='fwd', mat_preload=np.zeros_like(d['in0'])))
        staged = r['mat_out']
        model = fc.apply32(d['in0'], d['in1'], d['coef'])
        mat_ulps = float(np.max(np.abs(staged.astype(np.float64) - model) / fc.ulp(np.maximum(np.abs(model), 2.0 ** -20))))
        ref = cc.conv_acc(staged, d['w'], np.float64)
        c32 = cc.chain32(staged, d['w'])
    return name, {s: (cc.rel_rms(r['out'], ref, ax), cc.rel_rms(c32, ref, ax)) for s, ax in cc.SLICES.items()}, mat_ulps


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('cid', list(RANDOM_CASES))
def test_random_conv_matches_float64_within_twice_a_float32_chain(handle, cid, precision):
    """Measured on an MI355X: profiles/conv_fused/accuracy.json."""
    name, st, mat_ulps = measure_random(handle(precision), cid)
    print(f'{cid} {precision}: {name}; write-through against the float32 model: {mat_ulps} ulp')
    for s, (e, ec) in st.items():
        r = np.asarray(e / ec)
        print(f'  {s}: E kernel {np.max(e):.3g} (max), E chain32 {np.max(ec):.3g} (max), ratio max {r.max():.3f} median {np.median(r):.3f} over {r.size} slices')
    if mat_ulps is not None:   # fmaf is one rounding, the model's float64 route at most one more in a tie: 1 ulp
        assert mat_ulps <= 1.0, f'{cid} {precision}: the write-through is {mat_ulps} ulp from relu(fmaf(a, y, b) [+ x])'
    for s, (e, ec) in st.items():
        assert np.all(e <= BAR * ec), f'{cid} {precision} {s}: E = {np.max(e / ec):.3f} x chain32 (bar {BAR}), {name}'


def measure_ill(hl):
    x, wt = fc.ill_conditioned(**ILL)
    r, name = hl.debug_conv_fused(dict(weight=wt, in0=x, stat='fwd'))
    y = r['out']
    G = int(ran(name)['G'])
    v64 = y.astype(np.float64).var(axis=(0, 2, 3))
    ratio = y.astype(np.float64).mean(axis=(0, 2, 3)) ** 2 / v64
    var_k = fc.bn_fwd(r['part'], np.ones(ILL['cout'], np.float32), np.zeros(ILL['cout'], np.float32), y.size // ILL['cout'])['var']
    return name, ratio, rel_rms_over_channels(var_k, v64), rel_rms_over_channels(fc.var_pivot32(y, G), v64), rel_rms_over_channels(fc.var_naive32(y, G), v64)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_pivoted_partials_keep_the_variance_of_an_ill_conditioned_output(handle, precision):
    """The variance from the kernel's own partials against the float64 variance of the kernel's own output; the yardstick is a numpy float32 model of the
    pivoted sums (one running float32 sum per group), the bar twice its error (rms over the channels of the relative error).  A naive float32
    E[y^2] - mean^2 misses that bar by orders of magnitude on the same data (tests/test_conv_fused_host.py)."""
    name, ratio, e_k, e_model, e_naive = measure_ill(handle(precision))
    print(f'{precision} {name}: mean^2 / var {ratio.min():.3g} .. {ratio.max():.3g}; E kernel {e_k:.3g}, E pivot model {e_model:.3g}, E naive model {e_naive:.3g}')
    assert (ratio > 3e5).all()
    assert e_k <= 2.0 * e_model, f'{precision}: E = {e_k:.3g}, {e_k / e_model:.2f} x the float32 pivot model (bar 2)'
    assert e_naive > 2.0 * e_model


# ------------------------------------------------------------------------------------------ d. the write-through and k_lc_apply: the same bits
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('B,C,h,w', [(3, 5, 3, 3), (3, 21, 5, 7), (2, 33, 15, 15)])
def test_bnres_write_through_is_k_lc_apply_bit_for_bit(handle, precision, B, C, h, w):
    rs = np.random.RandomState(B * C * h)
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    y, res, coef = f(rs.randn(B, C, h, w)), f(rs.uniform(0, 1, (B, C, h, w))), f(np.stack([rs.uniform(0.5, 1.5, C), rs.randn(C) * 0.5, np.zeros(C)]))
    wt = f(rs.randn(4, C, 3, 3) * 0.1)
    hl = handle(precision)
    r, name = hl.debug_conv_fused(dict(weight=wt, in0=y, in1=res, coef=coef, in_mode='bnres', stat='fwd', mat_preload=np.full(y.shape, np.nan, np.float32)))
    a, aname = hl.debug_conv_fused(dict(y=y, res=res, coef=coef[:2]), mode='apply')
    check_ran(aname, 'apply', build='k_lc_apply', n=y.size, C=C, hw=h * w, res=1)
    if (B, C, h, w) != (2, 33, 15, 15):
        assert y.size % 4 != 0 and (h * w) % 2 == 1 and C % 16 != 0   # the scalar tail, an odd plane, channels off 16
    assert r['mat_out'].tobytes() == a['out'].tobytes(), f'{precision} {name} | {aname}: {fc.first_difference(r["mat_out"], a["out"], POS)}'
    assert 0.05 < (a['out'] == 0).mean() < 0.9
    assert (np.abs(a['out'].astype(np.float64) - fc.apply32(y, res, coef)) <= fc.ulp(np.maximum(fc.apply32(y, res, coef), 2.0 ** -20))).all()
    b, _ = hl.debug_conv_fused(dict(y=y, res=None, coef=coef[:2]), mode='apply')   # and without a residual: relu(fmaf(a, y, b))
    assert (np.abs(b['out'].astype(np.float64) - fc.apply32(y, None, coef)) <= fc.ulp(np.maximum(fc.apply32(y, None, coef), 2.0 ** -20))).all()


# ------------------------------------------------------------------------------------------ e. reproducibility, hygiene, refusals
def test_two_calls_give_the_same_bits(handle):
    for precision in PRECISIONS:
        for cid in ('bnres_9x9', 'bnbwd_9x9'):
            d = _random_data(cid)
            job = dict(weight=d['w'], in0=d['in0'], in1=d['in1'], coef=d['coef'], in_mode='bnres', stat='fwd', mat_preload=np.zeros_like(d['in0'])) if cid == 'bnres_9x9' else \
                dict(weight=fc.dgrad_weight(d['w']), direction=1, in0=d['in0'], in1=d['in1'], coef=d['coef'], in_mode='bnbwd', skip=d['skip'], mask=d['skip'], partner='mask', stat='bwd')
            (r0, n0), (r1, n1) = handle(precision).debug_conv_fused(job), handle(precision).debug_conv_fused(job)
            assert n0 == n1 and sorted(r0) == sorted(r1)
            for k in r0:
                assert np.asarray(r0[k]).tobytes() == np.asarray(r1[k]).tobytes(), (precision, cid, k)


def test_a_burst_of_hook_calls_leaves_the_update_alone():
    from test_gpu_conv_learner import _batch, _hip, _net, _ring

    dev = torch.device('cuda', 0)
    net, A = _net(9, 16, 2, 4, 77, dev)
    rs = np.random.RandomState(9)
    B = 6
    tr = _batch(rs, B, (4, 9, 9), A)
    w = torch.from_numpy(rs.uniform(0.3, 1.0, B).astype(np.float32)).to(dev)
    hl = _hip(net, dev, B)
    state = lambda: (hl.grad_flat.clone(), hl.params.clone())  # noqa: E731
    hl.grad(_ring(tr, dev), None, w, B)
    g0, p0 = state()
    d, refs = forward_refs('g3x3', 'S', 'bnres_mat')
    ops = fc.finalize_operands(1, 6)
    for i, wt, ref in refs:
        hl.debug_conv_fused(fwd_job(d, wt, finalize='fwd', gamma=ops['gamma'], beta=ops['beta'], running_mean=ops['running_mean'], running_var=ops['running_var'], num_batches=0))
    dg = fc.dgrad_case('g3x3', 'S')
    hl.debug_conv_fused(dgrad_job(dg, dg['draws'][0][0], 'second_conv', finalize='bwd', gamma=ops['gamma'], save=ops['save'], dgamma=ops['dgamma'], dbeta=ops['dbeta'], accumulate=True))
    hl.debug_conv_fused(dict(y=d['in0'], res=d['in1'], coef=d['coef'][:2]), mode='apply')
    g1, p1 = state()
    assert torch.equal(g0, g1) and torch.equal(p0, p1)   # the hook wrote nothing of the handle's
    hl.grad(_ring(tr, dev), None, w, B)
    g2, _ = state()
    assert g0.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes()   # and the next update computes the same gradient bytes
    hl.close()


def test_refusals(handle):
    from muzero_amd import hip_learner as hlm

    hl = handle()
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    ok = dict(weight=z(4, 4, 3, 3), in0=z(2, 4, 3, 3))
    hl.debug_conv_fused(dict(ok))
    coef = z(3, 4)
    bn = dict(gamma=z(4), beta=z(4))
    bad = [
        (dict(ok, stat='fwd', skip=z(2, 4, 3, 3)), 'launch_ops refused'),          # a forward-statistics conv carries no skip ...
        (dict(ok, stat='fwd', mask=z(2, 4, 3, 3)), 'launch_ops refused'),          # ... and no mask: launch_ops flags it, nothing is launched
        (dict(ok, in_mode='bnrelu'), 'inconsistent arguments: coef'),
        (dict(ok, coef=coef), 'inconsistent arguments: coef'),
        (dict(ok, in_mode='bnres', coef=coef), 'inconsistent arguments: in1'),
        (dict(ok, in1=z(2, 4, 3, 3)), 'inconsistent arguments: in1'),
        (dict(ok, mat_preload=z(2, 4, 3, 3)), 'write-through'),
        (dict(ok, mcoef=z(2, 4)), 'mcoef without mask'),
        (dict(ok, partner='mask', stat='bwd'), 'partner_is_mask needs mask'),
        (dict(ok, stat='bwd'), 'ST_BWD needs a partner'),
        (dict(ok, partner=z(2, 4, 3, 3)), 'ST_BWD needs a partner'),
        (dict(ok, finalize='fwd', **bn), 'finalize 1 follows ST_FWD'),
        (dict(ok, stat='fwd', finalize='bwd', gamma=z(4), save=z(2, 4)), 'finalize 1 follows ST_FWD'),
        (dict(weight=z(4, 4, 3, 3), in0=z(1, 4, 16, 16)), 'bad shape'),
    ]
    for job, pat in bad:
        with pytest.raises(hlm.LearnerError, match='mzl_debug_conv_fused.*' + pat):
            hl.debug_conv_fused(job)
    with pytest.raises(hlm.LearnerError, match='share in_mode and finalize'):
        hl.debug_conv_fused(dict(ok), mode='pair', second=dict(ok, in_mode='bnrelu', coef=coef))
    with pytest.raises(hlm.LearnerError, match="mode 'pair' needs"):
        hl.debug_conv_fused(dict(ok), mode='pair')
    with pytest.raises(hlm.LearnerError, match='does not fit weight'):
        hl.debug_conv_fused(dict(weight=z(4, 5, 3, 3), in0=z(2, 4, 3, 3)))
    # null pointers, an MLP handle and an Atari handle, at the ABI itself
    lib = hlm.load_library()
    name = hlm.C.c_char_p()
    call = hlm.MzlFusedCall()
    call.mode, call.batch, call.h, call.w = 0, 1, 3, 3
    call.conv[0].cin = call.conv[0].cout = 4
    assert lib.mzl_debug_conv_fused(hl._h, hlm.C.byref(call), hlm.C.byref(name)) == -1 and 'mzl_debug_conv_fused: null argument' in lib.mzl_last_error().decode()
    assert lib.mzl_debug_conv_fused(hl._h, None, hlm.C.byref(name)) == -1 and 'mzl_debug_conv_fused: null argument' in lib.mzl_last_error().decode()
    dev = torch.device('cuda', 0)
    mlp = hlm.HipLearner(build_mlp(mlp_case('tiny')).to(dev), dev, 5, 4, lr=1e-3)
    with pytest.raises(hlm.LearnerError, match='mzl_debug_conv_fused: needs a conv-net learner'):
        mlp.debug_conv_fused(dict(ok))
    mlp.close()
    at = hlm.HipLearner(build_conv(conv_case('atari_s')).to(dev), dev, 5, 2, lr=1e-3)
    with pytest.raises(hlm.LearnerError, match='mzl_debug_conv_fused: board nets only'):
        at.debug_conv_fused(dict(ok))
    at.close()
    # a refusal leaves the handle as it was: the same call, the same name and bits
    (r0, n0), (r1, n1) = hl.debug_conv_fused(dict(ok)), hl.debug_conv_fused(dict(ok))
    assert n0 == n1 and r0['out'].tobytes() == r1['out'].tobytes()


if __name__ == '__main__':  # python tests/test_gpu_conv_fused.py <out.json>: the errors of every random case, as the tests measure them
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    result = {'statistic': 'rms(out - conv64) / rms(conv64) of the conv of the staged operand; ratio = kernel / chain32 (a sequential float32 chain)', 'bar': BAR, 'cases': {},
              'ill_conditioned': {'statistic': 'rms over the channels of |var - var64| / var64, var64 = the float64 variance of the kernel\'s own output', 'bar': 2.0, 'shape': ILL}}
    for prec in PRECISIONS:
        h_ = _make(prec)
        for cid in RANDOM_CASES:
            name_, st_, mu = measure_random(h_, cid)
            entry = result['cases'].setdefault(cid, {'shape': dict(zip(('mode', 'h', 'w', 'c_in', 'c_out', 'batch'), RANDOM_CASES[cid]))})
            worst = max(float(np.max(st_[s][0] / st_[s][1])) for s in ('channel', 'pixel'))
            entry[prec] = {'ran': name_, 'chain32': float('%.4g' % float(st_['whole'][1])), 'kernel': float('%.4g' % float(st_['whole'][0])),
                           'ratio': round(float(st_['whole'][0] / st_['whole'][1]), 4), 'worst_slice_ratio': round(worst, 4), 'write_through_ulps_from_model': mu}
        name_, ratio_, e_k_, e_m_, e_n_ = measure_ill(h_)
        result['ill_conditioned'][prec] = {'ran': name_, 'mean2_over_var': [float('%.4g' % ratio_.min()), float('%.4g' % ratio_.max())], 'kernel': float('%.4g' % e_k_),
                                           'pivot_model_float32': float('%.4g' % e_m_), 'naive_model_float32': float('%.4g' % e_n_), 'ratio': round(e_k_ / e_m_, 4)}
        h_.close()
    with open(sys.argv[1], 'w') as f_:
        json.dump(result, f_, indent=1)
        f_.write('\n')
    print(json.dumps(result, indent=1))
