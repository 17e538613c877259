"""The references and data of tests/test_gpu_conv_fused.py, checked without a GPU (tests/conv_fused_cases.py):
1. the reference chain conv -> train-mode BatchNorm -> ReLU -> conv -> BatchNorm -> + residual -> ReLU -> conv, built from the pieces the GPU file compares
   the kernels with (staging transforms, pivoted partials, both finalizes, the data-gradient epilogue), is float64 autograd's, forward and backward;
2. the integer classes stay exact in float32 in any order on every case the GPU file runs, and the cases have the properties they are there for;
3. every deliberate mistake of cases.MUTATIONS changes the reference on every case where it can occur;
4. on the ill-conditioned data a naive float32 E[y^2] - mean^2 misses the bar that the pivoted model sets."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_fused_cases as fc
import conv_layer_cases as cc
from helpers import REPO

t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))  # noqa: E731


# ------------------------------------------------------------------------------------------ the hook's place in the ABI
def test_hook_is_exported_not_declared_and_its_argument_block_is_mirrored():
    from muzero_amd import hip_learner as hl

    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'mzlearner.h')).read(), flags=re.S)
    assert 'mzl_debug_conv_fused' not in text and 'mzl_debug_conv_fused' not in hl.ABI_SYMBOLS
    host = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'mz_learn_conv_host.h')).read()
    for struct, mirror in (('mzl_fused_conv', hl.MzlFusedConv), ('mzl_fused_call', hl.MzlFusedCall)):
        body = re.sub(r'//[^\n]*', '', re.search(r'struct\s+%s\s*\{(.*?)\n\};' % struct, host, flags=re.S).group(1))
        names = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                names += [re.sub(r'\[\d+\]', '', n).strip(' *') for n in decl.split(None, 2 if decl.startswith('const') else 1)[-1].split(',')]
        assert names == [n for n, _ in mirror._fields_], (struct, names)
    assert C.sizeof(hl.MzlFusedConv) == 23 * 8 + 8 * 4 and C.sizeof(hl.MzlFusedCall) == 8 * 4 + 2 * C.sizeof(hl.MzlFusedConv)
    enums = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'mz_learn_conv.h')).read()
    assert 'enum { IN_IDENT = 0, IN_BNRELU = 1, IN_BNBWD = 2, IN_BNRES = 3 }' in enums and 'enum { ST_NONE = 0, ST_FWD = 1, ST_BWD = 2 }' in enums
    assert hl.IN_MODES == dict(ident=0, bnrelu=1, bnbwd=2, bnres=3) and hl.STAT_MODES['fwd'] == 1 and hl.STAT_MODES['bwd'] == 2
    assert re.search(r'extern "C" int mzl_debug_conv_fused\(', open(os.path.join(REPO, 'muzero_amd', 'csrc', 'learner.hip')).read())


def test_conv_geom_is_make_geoms_choice_for_every_case():
    for key, (h, w, B, ci, co, no_side, exp) in fc.GEOMS.items():
        npt, G = fc.conv_geom(h, w, B)
        assert (npt, G, -(-B // G)) == (exp['NPT'], exp['G'], exp['groups']), key
        assert exp['SIDE'] == (15 if (h, w, G, npt) == (15, 15, 1, 15) and not no_side else 0), key
        assert exp.get('z', 1) == -(-(-(-co // 16)) // 4), key
    g = fc.GEOMS
    assert g['g3x3'][6]['G'] > 1 and g['g3x3'][6]['groups'] >= 3 and g['g3x3'][2] % g['g3x3'][6]['G'] != 0 and 9 % 4 != 0   # a short last group; quads straddle images
    assert 36 % 4 == 0 and 35 % 4 != 0 and 49 % 16 != 0 and 169 % 16 != 0
    assert g['g3x3_c72'][4] > 64 and g['g6x6_c24'][4] % 16 != 0 and g['g6x6'][4] < 16 and g['g6x6_c24'][3] % 16 != 0 and g['g9x9'][3] % 16 != 0 and g['g6x6_c24'][3] > 32


# ------------------------------------------------------------------------------------------ 1. the reference chain is autograd's
def test_reference_chain_is_float64_autograd_forward_and_backward():
    rs = np.random.RandomState(11)
    B, c0, c1, c3, h, w, G = 5, 4, 4, 3, 4, 5, 2   # (a residual block keeps its channel count: c0 -> c1 == c0 -> c0, then a consumer conv c0 -> c3)
    x0 = np.maximum(rs.randn(B, c0, h, w), 0.0)
    w1, w2, w3 = rs.randn(c1, c0, 3, 3) * 0.3, rs.randn(c0, c1, 3, 3) * 0.3, rs.randn(c3, c0, 3, 3) * 0.3
    gam1, bet1, gam2, bet2 = rs.uniform(0.5, 1.5, c1), rs.randn(c1) * 0.3, rs.uniform(0.5, 1.5, c0), rs.randn(c0) * 0.3
    rm1, rv1, rm2, rv2 = rs.randn(c1), rs.uniform(0.5, 2, c1), rs.randn(c0), rs.uniform(0.5, 2, c0)
    gy3 = rs.randn(B, c3, h, w)
    N = B * h * w
    # ---- torch
    xt = t64(x0).requires_grad_(True)
    bn1, bn2 = torch.nn.BatchNorm2d(c1).double(), torch.nn.BatchNorm2d(c0).double()
    for bn, g, b, rm, rv in ((bn1, gam1, bet1, rm1, rv1), (bn2, gam2, bet2, rm2, rv2)):
        bn.weight.data, bn.bias.data, bn.running_mean.data, bn.running_var.data = t64(g), t64(b), t64(rm).clone(), t64(rv).clone()
        bn.train()
    ty1 = F.conv2d(xt, t64(w1), padding=1)
    tz1 = torch.relu(bn1(ty1))
    ty2 = F.conv2d(tz1, t64(w2), padding=1)
    tout = torch.relu(bn2(ty2) + xt)
    ty3 = F.conv2d(tout, t64(w3), padding=1)
    (ty3 * t64(gy3)).sum().backward()
    # ---- the references, in the update's order
    close = lambda a, b: np.testing.assert_allclose(a, b.detach().numpy() if torch.is_tensor(b) else b, rtol=1e-12, atol=1e-12)  # noqa: E731
    y1 = cc.conv_acc(x0, w1, np.float64)
    f1 = fc.bn_fwd(fc.partials_fwd(y1, G), gam1, bet1, N, rm1, rv1)
    coef1 = np.stack([f1['a'], f1['b'], np.zeros(c1)])
    z1 = fc.stage('bnrelu', y1, None, coef1)
    y2 = cc.conv_acc(z1, w2, np.float64)
    f2 = fc.bn_fwd(fc.partials_fwd(y2, G), gam2, bet2, N, rm2, rv2)
    coef2 = np.stack([f2['a'], f2['b'], np.zeros(c0)])
    out = fc.mat_out('bnres', y2, x0, coef2)
    y3 = cc.conv_acc(fc.stage('bnres', y2, x0, coef2), w3, np.float64)
    for mine, theirs in ((y1, ty1), (z1, tz1), (y2, ty2), (out, tout), (y3, ty3), (f1['running_mean'], bn1.running_mean), (f1['running_var'], bn1.running_var),
                         (f2['running_mean'], bn2.running_mean), (f2['running_var'], bn2.running_var)):
        close(mine, theirs)
    assert int(bn1.num_batches_tracked) == 1
    # backward: the consumer's data gradient masked by the block output (materialised: mask > 0), statistics against y2
    t2 = fc.epilogue(cc.conv_acc(gy3, fc.dgrad_weight(w3), np.float64), mask=out)
    b2 = fc.bn_bwd(fc.partials_bwd(t2, y2, G), gam2, np.stack([f2['mean'], f2['invstd']]), N)
    dy2 = fc.stage('bnbwd', t2, y2, np.stack([b2['c1'], b2['c2'], b2['c3']]))
    # the second conv's data gradient, masked by relu(a1 y1 + b1) never materialised (mcoef), the partner IS the mask buffer
    t1 = fc.epilogue(cc.conv_acc(dy2, fc.dgrad_weight(w2), np.float64), mask=y1, mcoef=coef1[:2])
    b1 = fc.bn_bwd(fc.partials_bwd(t1, y1, G), gam1, np.stack([f1['mean'], f1['invstd']]), N)
    dy1 = fc.stage('bnbwd', t1, y1, np.stack([b1['c1'], b1['c2'], b1['c3']]))
    # the first conv's data gradient + the skip gradient (the block input is no ReLU output of this tower here: no mask)
    dx = fc.epilogue(cc.conv_acc(dy1, fc.dgrad_weight(w1), np.float64), skip=t2)
    for mine, theirs in ((dx, xt.grad), (b1['dgamma'], bn1.weight.grad), (b1['dbeta'], bn1.bias.grad), (b2['dgamma'], bn2.weight.grad), (b2['dbeta'], bn2.bias.grad)):
        close(mine, theirs)
    assert 0.2 < (z1 == 0).mean() < 0.8 and 0.1 < (out == 0).mean() < 0.9
    # accumulate adds to what the slots hold
    acc = fc.bn_bwd(fc.partials_bwd(t1, y1, G), gam1, np.stack([f1['mean'], f1['invstd']]), N, dgamma0=rm1, dbeta0=rv1, accumulate=True)
    close(acc['dgamma'], b1['dgamma'] + rm1)
    close(acc['dbeta'], b1['dbeta'] + rv1)
    # k_lc_apply's float32 model against float64
    c32 = coef2.astype(np.float32)
    np.testing.assert_allclose(fc.apply32(y2.astype(np.float32), x0.astype(np.float32), c32), fc.mat_out('bnres', y2.astype(np.float32), x0.astype(np.float32), c32), rtol=3e-7, atol=3e-7)


# ------------------------------------------------------------------------------------------ 2. the integer cases
@functools.lru_cache(maxsize=None)
def forward_refs(key, cls, combo):
    """[(draw index, weight, staged operand, int64 output)] of one forward run: computed once, shared, never written to."""
    d = fc.forward_case(key, cls, combo)
    refs = [(i, wt, cc.conv_acc(d['target'], wt, np.int64)) for i, (wt, _) in enumerate(d['draws'])]
    return d, refs


@pytest.mark.parametrize('key', list(fc.GEOMS))
def test_integer_cases_are_exact_in_float32_and_have_their_properties(key):
    h, w, B, ci, co, _, exp = fc.GEOMS[key]
    G, npt = exp['G'], exp['NPT']
    for cls in fc.CLASSES_OF[key]:
        for combo, (mode, mat) in fc.FWD_COMBOS.items():
            if mat:
                continue
            d, refs = forward_refs(key, cls, combo)
            staged = fc.stage(mode, d['in0'], d['in1'], d['coef'])
            assert np.array_equal(staged, d['target']) and np.array_equal(staged, np.rint(staged))
            if mode != 'ident':
                pre = fc.stage(mode, d['in0'], d['in1'], d['coef'], pre=True)
                assert 0.25 < (pre < 0).mean() < 0.75 if cls != 'S' else 0.2 < (pre < 0).mean() < 0.6, (key, cls, combo, (pre < 0).mean())   # the ReLU zeroes about a third and more
            assert cc.covered(d['draws']).all() and cc.im2col((staged != 0).astype(np.float64)).any(axis=0).all(), (key, cls, combo)  # every (channel, tap) still meets a nonzero value
            for i, wt, ref in refs:
                plain, terms = cc.int_bounds(staged.astype(np.float32), wt, np.zeros(co, np.float32))
                assert plain < 2 ** 23 and terms < 2 ** 24, (key, cls, combo, i)
                if cls == 'S':
                    assert np.abs(staged).max() <= fc.S_MAX and set(np.unique(wt)) <= {-1.0, 0.0, 1.0} and (wt != 0).reshape(co, -1).sum(1).max() <= 27 and np.abs(ref).max() <= 81
                    part = fc.partials_fwd(ref, G)
                    assert (part[:, :co, 0] != 0).all(), (key, combo, i, 'a zero pivot')   # a padding slot counted by mistake then adds -p, not 0
                    assert part[:, :, 2].max() < 2 ** 24 and np.abs(part[:, :, 1]).max() < 2 ** 24 and 240 * 162 ** 2 < 2 ** 24
                    assert (part[:, co:] == 0).all() and part[:, :co, 3].sum(0).tolist() == [B * h * w] * co
        d = fc.dgrad_case(key, cls)
        staged = fc.stage('bnbwd', d['in0'], d['in1'], d['coef'])
        assert np.array_equal(staged, d['target']) and cc.covered(d['draws']).all()
        e = d['epi']
        v = e['mcoef'][0].reshape(1, -1, 1, 1) * e['mask'].astype(np.float64) + e['mcoef'][1].reshape(1, -1, 1, 1)
        assert (e['mask'] == 0).any(axis=(0, 2, 3)).all() and (v == 0).any(axis=(0, 2, 3)).all() and (v > 0).any() and (v < 0).any()   # exact zeros of both kinds, in every channel
        for i, (wt, _) in enumerate(d['draws']):
            plain, terms = cc.int_bounds(staged.astype(np.float32), wt, np.full(co, 4.0, np.float32))   # (|skip| <= 4 rides as a bias)
            assert plain < 2 ** 23 and terms < 2 ** 24, (key, cls, 'dgrad', i)
            if cls == 'S':
                for combo in ('second_conv', 'first_conv'):
                    t, part = fc.dgrad_reference(d, wt, combo, G)
                    assert np.abs(t).max() <= 85 and np.abs(part).max() < 2 ** 24 and G * h * w * 85 * 3 < 2 ** 24


# ------------------------------------------------------------------------------------------ 3. every deliberate mistake changes the reference
def test_every_mutation_changes_the_reference_wherever_it_can_occur():
    seen = set()
    for key, (h, w, B, ci, co, _, exp) in fc.GEOMS.items():
        G, npt = exp['G'], exp['NPT']
        d, refs = forward_refs(key, 'S', 'bnres')
        for i, wt, ref in refs:
            good = fc.partials_fwd(ref, G)
            for bug, can in (('pad_slot_counted', npt * 16 > G * h * w), ('short_group_full', B % G != 0), ('n_full_for_short', B % G != 0), ('pivot_wrong_image', G > 1)):
                if can:
                    bad = fc.partials_fwd(ref, G, npt=npt, bug=bug)
                    assert (bad[:, :co] != good[:, :co]).any(axis=(0, 2)).all(), (key, i, bug)  # (in every channel)
                    seen.add(bug)
        for combo in ('bnrelu', 'bnres'):
            d, refs = forward_refs(key, 'S', combo)
            good = fc.mat_out(d['mode'], d['in0'], d['in1'], d['coef'])
            assert not np.array_equal(good, fc.mat_out(d['mode'], d['in0'], d['in1'], d['coef'], bug='relu_dropped_mat'))
            seen.add('relu_dropped_mat')
            if combo == 'bnres':
                assert all(not np.array_equal(cc.conv_acc(fc.stage('bnres', d['in0'], d['in1'], d['coef'], bug='residual_dropped'), wt, np.float64), ref) for _, wt, ref in refs)
                seen.add('residual_dropped')
        d = fc.dgrad_case(key, 'S')
        for i, (wt, _) in enumerate(d['draws']):
            for bug, combos in (('c3_dropped', ('bare',)), ('in1_as_in0', ('bare',)), ('skip_after_mask', ('first_conv',)), ('mask_ge', ('first_conv', 'second_conv')),
                                ('mcoef_ignored', ('second_conv',)), ('partner_from_mask', ('first_conv',))):
                for combo in combos:
                    (t, p), (tb, pb) = fc.dgrad_reference(d, wt, combo, G), fc.dgrad_reference(d, wt, combo, G, bug=bug)
                    assert not np.array_equal(p, pb) if bug == 'partner_from_mask' else not np.array_equal(t, tb), (key, i, bug, combo)
                    seen.add(bug)
    ops = fc.finalize_operands(5, fc.FINALIZE_C)
    for groups in fc.FINALIZE_GROUPS:
        pf, pb = fc.finalize_parts(groups, groups, fc.FINALIZE_C, 'fwd'), fc.finalize_parts(groups + 1, groups, fc.FINALIZE_C, 'bwd')
        kw = dict(gamma=ops['gamma'], beta=ops['beta'], count=groups * 72, running_mean=ops['running_mean'], running_var=ops['running_var'])
        good = fc.bn_fwd(pf, **kw)
        assert np.allclose(good['n'], groups * 72)
        assert (fc.bn_fwd(pf, bug='biased_running_var', **kw)['running_var'] != good['running_var']).all()
        kb = dict(gamma=ops['gamma'], save=ops['save'], count=groups * 72, dgamma0=ops['dgamma'], dbeta0=ops['dbeta'], accumulate=True)
        goodb = fc.bn_bwd(pb, **kb)
        assert (goodb['cancel'] > 2.0 ** -20).all(), groups   # s2 - mean s1 keeps its digits
        badb = fc.bn_bwd(pb, bug='accumulate_ignored', **kb)
        assert (badb['dgamma'] != goodb['dgamma']).all() and (badb['dbeta'] != goodb['dbeta'])[ops['dbeta'] != 0].all()
        seen |= {'biased_running_var', 'accumulate_ignored'}
        for unroll, kind in ((4, 'fwd'), (8, 'bwd')):   # a slice whose group count is no multiple of the unrolled loop's step has a tail
            if any(len(range(s, groups, 16)) % unroll for s in range(16)):
                a = fc.bn_fwd(pf, bug='group_past_unroll_dropped', **kw)['mean'] if kind == 'fwd' else fc.bn_bwd(pb, bug='group_past_unroll_dropped', **kb)['dbeta']
                assert (a != (good['mean'] if kind == 'fwd' else goodb['dbeta'])).all(), (groups, kind)
                seen.add('group_past_unroll_dropped')
    # the float64 sums follow the kernels' order (slices, then groups): another order gives other float64 bits on the long case
    pf = fc.finalize_parts(3001, 3001, fc.FINALIZE_C, 'fwd')
    V = pf[:, :, 0].astype(np.float64) * pf[:, :, 1]   # (p S1: 48-bit products; the float32 partials themselves add exactly in float64 in any order)
    assert (fc.slice_sums(V, 4) != fc.slice_sums(V, 4, bug='slice_order'))[:fc.FINALIZE_C].any()
    seen.add('slice_order')
    assert seen == set(fc.MUTATIONS), set(fc.MUTATIONS) - seen


# ------------------------------------------------------------------------------------------ 4. what the pivot is for
ILL = dict(seed=77, B=6, cin=8, cout=16, h=9, w=9)


def rel_rms_over_channels(v, ref):
    return float(np.sqrt((((np.asarray(v, np.float64) - ref) / ref) ** 2).mean()))


def test_naive_float32_variance_misses_the_bar_the_pivoted_model_sets():
    x, wt = fc.ill_conditioned(**ILL)
    y = cc.chain32(x, wt)
    v64 = y.astype(np.float64).var(axis=(0, 2, 3))
    ratio = y.astype(np.float64).mean(axis=(0, 2, 3)) ** 2 / v64
    assert (ratio > 3e5).all() and (ratio < 3e6).all(), ratio
    _, G = fc.conv_geom(ILL['h'], ILL['w'], ILL['B'])
    e_pivot, e_naive = rel_rms_over_channels(fc.var_pivot32(y, G), v64), rel_rms_over_channels(fc.var_naive32(y, G), v64)
    print(f'mean^2 / var {ratio.min():.3g} .. {ratio.max():.3g}: E pivot {e_pivot:.3g}, E naive {e_naive:.3g}')
    assert e_naive > 2.0 * e_pivot and e_naive > 100 * e_pivot
