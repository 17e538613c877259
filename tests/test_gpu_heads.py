"""The conv learner's head block (csrc/mz_learn_conv.h k_lch_conv, k_lch_bn, k_lch_loss, k_lch_bnb, k_lch_dx, k_lch_dw1, k_lch_dlin, k_lch_wsum, with
k_lc_pack_lin) alone, through mzl_debug_heads -- the update's own launch code on temporary buffers -- against the float64 model of
tests/heads_cases.py (which tests/test_heads_host.py holds to float64 autograd through the project's heads and loss).

a. Integer data: u, the pivoted partials and pivots, the ReLU pattern and dz's zeros equal the model; the heads' gradients equal the float32 step-order
   sum of the returned per-step partials; num_batches_tracked goes up by K; a second call returns the same bits.
b. Random data, stage by stage: every kernel output against the float64 model fed the KERNEL's own inputs (the previous kernels' outputs as returned).
   Statistic: rms(out - model) / rms(model) over a tensor of one group.  Bar: twice the same statistic of the float32 chain twin on the same inputs (a
   tensor of fewer than 64 elements: at least one correct rounding, 2^-24 of the model's rms, since a chain of so few samples can be exact by luck).
   The outputs that pass through expf / logf / sqrtf / a division, and the squared-error terms (logit - target cancels), are counted in float32 ulps of their natural scale instead (ULP_STAGES): the worst
   element's error, bar twice the chain's worst.  profiles/heads/accuracy.json holds chain, bar and kernel per stage and geometry
   (python tests/test_gpu_heads.py writes it).
c. End to end on edge data (targets at 0, around +-half and far outside the support, policy rows of mass 0 and 0.5, weights zero and 1e4 apart, rows
   repeated and out of order, logits near +-80, gamma = 0, a constant plane): loss, priorities, both tower gradients, every head gradient and the running
   statistics against the float64 model, bars from the float32 chain of the whole block in the same way (E2E_FLOOR says what the chain cannot show).
   A batch of one or two images is held to the larger of its own bar and that of the geometry's largest batch (rows_of).
d. Refusals."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import helpers  # noqa: F401  (puts the repository root on sys.path)
import heads_cases as hc

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
_LEARNERS = {}
NETS = {  # geometry -> (net kind, input shape, blocks, max_batch)
    'board3': ('board', (2, 3, 3), 1, 130), 'board5': ('board', (2, 5, 5), 1, 65), 'board15': ('board', (2, 15, 15), 1, 130), 'board15x16': ('board', (2, 15, 16), 1, 64),
    'board3_p40': ('board', (2, 3, 3), 1, 63), 'atari': ('atari', (4, 96, 96), 1, 65), 'atari301': ('atari', (4, 96, 96), 1, 64),
}
CASES = [(n, B) for n in sorted(hc.GEOMS) for B in hc.BATCHES[n]]
LAST = [(n, hc.BATCHES[n][-1]) for n in sorted(hc.GEOMS)]


def _learner(name):
    if name not in _LEARNERS:
        from muzero_amd.hip_learner import HipLearner
        from muzero_amd.network import MuZeroAtariNet, MuZeroBoardGameNet
        kind, shape, blocks, max_batch = NETS[name]
        g = hc.GEOMS[name]
        torch.manual_seed(3)
        net = MuZeroBoardGameNet(shape, g.A, blocks, g.P) if kind == 'board' else MuZeroAtariNet(shape, g.A, blocks, g.P, g.Sv, g.Sr)
        dev = torch.device('cuda', 0)
        _LEARNERS[name] = HipLearner(net.to(dev), dev, g.K, max_batch, lr=1e-3)
    return _LEARNERS[name]


@pytest.fixture(scope='module', autouse=True)
def _close_learners():
    yield
    for h in _LEARNERS.values():
        h.close()
    _LEARNERS.clear()


def run(name, case, skip=()):
    running = np.concatenate([np.concatenate([np.asarray(rm, f32), np.asarray(rv, f32)]) for rm, rv in case['running']])
    return _learner(name).debug_heads(case['F_pred'], case['F_rew'], hc.flat_params(case['heads']), running, case['nbt'], case['pi'], case['value'], case['reward'],
                                      case['idx'], case['w'], skip=skip)


def where(what, g, i, arr_idx, names):
    t, hd = divmod(i, 3)
    return f'{what}: {hc.HEAD_NAMES[hd]} head, step {t}, ' + ', '.join(f'{n} {int(v)}' for n, v in zip(names, arr_idx))


def worst(err):
    return np.unravel_index(int(np.argmax(err)), err.shape)


# ---- a. integer data ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,B', CASES)
def test_integer_data_is_exact_and_repeatable(name, B):
    g = hc.GEOMS[name]
    case = hc.integer_case(g, B, hc.case_seed(name, B))
    out, again = run(name, case), run(name, case)
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), f'{name} B={B}: {k} differs between two calls on the same data'
    ref = hc.model(case, g)
    for i, r in enumerate(ref['groups']):
        oc = r['u'].shape[1]
        for label, got, want, names in (('u', out['u'][i][:, :oc], r['u'], ('image', 'plane', 'position')),
                                        ('pivot', out['spiv'][i][:, :oc], r['piv'], ('image', 'plane')),
                                        ('forward partial', out['spart_fwd'][i][:, :oc], r['part'], ('image', 'plane', 'entry (sum, sum of squares)'))):
            bad = got.astype(f64) != want
            assert not bad.any(), where(f'{name} B={B} {label} is not the exact integer', g, i, worst(bad), names) + f': {got[worst(bad)]} for {want[worst(bad)]}'
        feat, dz = out['feat'][i][:, :oc * g.hw].reshape(B, oc, g.hw), out['dzb'][i][:, :oc]
        bad = (feat > 0) != (r['pre'] > 0)
        assert not bad.any(), where(f'{name} B={B} ReLU pattern', g, i, worst(bad), ('image', 'plane', 'position'))
        bad = ((feat > 0) == 0) & (dz != 0)
        assert not bad.any(), where(f'{name} B={B} dz is not zero behind a closed ReLU', g, i, worst(bad), ('image', 'plane', 'position'))
        assert np.isnan(out['u'][i][:, oc:]).all() and np.isnan(out['dzb'][i][:, oc:]).all(), f'{name}: a plane the head lacks was written'
    assert (out['nbt_out'] == case['nbt'] + g.K).all(), f'{name} B={B}: num_batches_tracked {out["nbt_out"]} from {case["nbt"]}, K = {g.K}'
    _wsum_is_step_order_sum(name, B, g, out)


def _wsum_is_step_order_sum(name, B, g, out):
    grads, parts = hc.split_params(out['grads'], g), hc.split_wpart(out['wpart'], g)
    for hd, hn in enumerate(hc.HEAD_NAMES):
        for k in ('w1', 'lw', 'lb'):
            s = np.zeros_like(parts[hd][0][k])
            for t in range(g.K):
                s = s + parts[hd][t][k]
            bad = s.view(np.uint32) != np.ascontiguousarray(grads[hd][k]).view(np.uint32)
            assert not bad.any(), f'{name} B={B}: {hn} d{k} is not the float32 step-order sum of the per-step partials at {worst(bad)}'


@pytest.mark.parametrize('name', ['board3', 'board15', 'atari'])
def test_a_plane_a_head_does_not_have_contributes_nothing(name):
    """k_lch_dx sums the policy's two planes and the value's one into dF_pred, the reward's one into dF_rew; the weights of a plane a head lacks are never
    staged.  With the Linear weights zero every real plane's du is exactly zero (dz = 0, so c2 = c3 = 0): dF must be exactly zero, not 0 x garbage.
    With only the prediction heads' Linear weights zero, dF_pred is zero and dF_rew is not."""
    g, B = hc.GEOMS[name], 3
    case = hc.random_case(g, B, 77)
    for zero in ((0, 1, 2), (1, 2)):
        c = dict(case, heads=[dict(p, lw=np.zeros_like(p['lw'])) if hd in zero else p for hd, p in enumerate(case['heads'])])
        out = run(name, c)
        bad = out['dF_pred'] != 0
        assert not bad.any(), f'{name}: dF_pred is not exactly zero at (step, image, channel, position) {worst(bad)}: {out["dF_pred"][worst(bad)]}'
        if 0 in zero:
            bad = out['dF_rew'] != 0
            assert not bad.any(), f'{name}: dF_rew is not exactly zero at (step, image, channel, position) {worst(bad)}: {out["dF_rew"][worst(bad)]}'
        else:
            assert np.isfinite(out['dF_rew']).all() and (out['dF_rew'] != 0).any()


# ---- b. stage by stage ------------------------------------------------------------------------------------------------------------------------------------
def rel_rms(x, ref):
    x, ref = np.asarray(x, f64), np.asarray(ref, f64)
    d = float(np.sqrt(np.mean((x - ref) ** 2))) if ref.size else 0.0
    s = float(np.sqrt(np.mean(ref ** 2))) if ref.size else 0.0
    return d / s if s > 0 else (0.0 if d == 0 else float('inf'))


def ulps(x, ref, scale):
    """worst |x - ref| in float32 ulps of `scale` (broadcast against ref), where scale > 0; elsewhere x must equal ref exactly."""
    x, ref = np.asarray(x, f64), np.asarray(ref, f64)
    scale = np.broadcast_to(np.asarray(scale, f64), ref.shape)
    live = scale > 0
    assert (x[~live] == ref[~live]).all(), 'an element whose scale is zero (zero weight) is not exactly the model\'s'
    return float((np.abs(x - ref)[live] / hc.ulp(scale[live])).max()) if live.any() else 0.0


ULP_STAGES = ('k_lch_bn invstd', 'k_lch_loss dlogit (squared error)', 'k_lch_loss lpart (squared error)', 'k_lch_loss priority (squared error)', 'k_lch_bnb dgamma',
              'k_lch_bnb dbeta', 'k_lch_bnb loss', 'k_lch_loss softmax (dlogit)', 'k_lch_loss 2-hot weights (dlogit at the target bins)', 'k_lch_loss lse (lpart)',
              'k_lch_loss signed_parabolic (priority)')


def stage_rows(name, B, case, out):
    """[(stage, group or -1, kernel, chain, bar)]: every kernel's outputs against the float64 model fed that kernel's inputs as the hook returned them."""
    g = hc.GEOMS[name]
    H = hc.heads(g)
    rows = []

    def add(stage, i, got, m64, m32):
        ek, ec = rel_rms(got, m64), rel_rms(m32, m64)
        floor = 2.0 ** -24 if np.size(m64) < 64 else 0.0
        rows.append((stage, i, ek, ec, 2.0 * max(ec, floor)))

    def add_ulp(stage, i, got, m64, m32, scale):
        rows.append((stage, i, ulps(got, m64, scale), ulps(m32, m64, scale), 2.0 * ulps(m32, m64, scale)))

    running = [(np.asarray(rm, f32), np.asarray(rv, f32)) for rm, rv in case['running']]
    running64 = [(np.asarray(rm, f64), np.asarray(rv, f64)) for rm, rv in case['running']]
    coef, save = out['coef'], out['save']
    du_k = [None] * (3 * g.K)
    for t in range(g.K):
        for hd, (oc, n, kind, src, _) in enumerate(H):
            i, p, F = 3 * t + hd, case['heads'][hd], case[src][t]
            u = out['u'][i][:, :oc]
            add('k_lch_conv u', i, u, hc.st_conv(F, p['w1'], f64), hc.st_conv(F, p['w1'], f32))
            piv = out['spiv'][i][:, :oc]
            assert (piv == u[..., 0]).all(), where(f'{name} B={B} pivot is not u at position 0', g, i, worst(piv != u[..., 0]), ('image', 'plane'))
            part = out['spart_fwd'][i][:, :oc]
            add('k_lch_conv pivoted partials', i, part, hc.st_pivot(u, piv, f64), hc.st_pivot(u, piv, f32))
            # k_lch_bn on the kernel's partials; the running statistics chain through the steps (model: the model's own previous step)
            b64 = hc.st_bn(part, piv, g.hw, p['gamma'], p['beta'], *running64[hd], f64)
            b32 = hc.st_bn(part, piv, g.hw, p['gamma'], p['beta'], *running[hd], f32)
            running64[hd], running[hd] = (b64['rm'], b64['rv']), (b32['rm'], b32['rv'])
            a, b = coef[i, :oc, 0], coef[i, :oc, 1]
            add_ulp('k_lch_bn invstd', i, save[i, :oc, 1], b64['invstd'], b32['invstd'], b64['invstd'])
            add('k_lch_bn mean', i, save[i, :oc, 0], b64['mean'], b32['mean'])
            add('k_lch_bn a', i, a, b64['a'], b32['a'])
            add('k_lch_bn b', i, b, b64['b'], b32['b'])
            # k_lch_loss: feat from (u, a, b); the losses from feat; dz from dlogit; the backward partials from dz and u
            feat = out['feat'][i][:, :oc * g.hw]
            add('k_lch_loss feat', i, feat, hc.st_feat(u, a, b, f64).reshape(B, -1), hc.st_feat(u, a, b, f32).reshape(B, -1))
            sc, pi = hc.st_targets(case, g, hd, t)
            lg64 = hc.st_logits(feat, p['lw'], p['lb'], f64)
            l64 = hc.st_loss(lg64, kind, sc, pi, case['w'], g.K, f64, S=n)
            l32 = hc.st_loss(hc.st_logits(feat, p['lw'], p['lb'], f32), kind, sc, pi, case['w'], g.K, f32, S=n)
            dl = out['dlogit'][i][:, :n]
            gs = (case['w'].astype(f64) / (B * g.K))[:, None]
            if kind == 0:
                # d = logit - target cancels, and so can the logit's own sum: the error is that sum's, so it is counted in ulps of the sum of the
                # absolute terms (or the target, if larger), which no sample makes small by chance -- not relative to d or to the logit
                top = np.maximum(np.abs(feat.astype(f64)) @ np.abs(p['lw'].astype(f64)).T[:, 0] + np.abs(f64(p['lb'][0])), np.abs(sc.astype(f64)))
                add_ulp('k_lch_loss dlogit (squared error)', i, dl, l64['dlogit'], l32['dlogit'], (2.0 * gs[:, 0] * top)[:, None])
                add_ulp('k_lch_loss lpart (squared error)', i, out['lpart'][i], l64['lpart'], l32['lpart'], case['w'].astype(f64) * top * top)
            else:
                sp = np.maximum(l64['target'].sum(1, keepdims=True), 1.0)
                add_ulp('k_lch_loss softmax (dlogit)', i, dl, l64['dlogit'], l32['dlogit'], np.broadcast_to(gs * sp, dl.shape))
                if kind == 2:
                    tb = l64['target'] > 0
                    rows.append(('k_lch_loss 2-hot weights (dlogit at the target bins)', i, ulps(dl[tb], l64['dlogit'][tb], np.broadcast_to(gs * sp, dl.shape)[tb]),
                                 ulps(l32['dlogit'][tb], l64['dlogit'][tb], np.broadcast_to(gs * sp, dl.shape)[tb]),
                                 2.0 * ulps(l32['dlogit'][tb], l64['dlogit'][tb], np.broadcast_to(gs * sp, dl.shape)[tb])))
                lscale = case['w'].astype(f64) * np.maximum(np.abs(l64['target'].sum(1) * l64['lse']), np.abs((l64['lpart'] / np.where(case['w'] == 0, 1, case['w'])) - l64['target'].sum(1) * l64['lse']))
                add_ulp('k_lch_loss lse (lpart)', i, out['lpart'][i], l64['lpart'], l32['lpart'], lscale)
            if hd == 2 and t == 0:
                if kind == 2:
                    add_ulp('k_lch_loss signed_parabolic (priority)', i, out['prio'], l64['prio'], l32['prio'], np.maximum(np.abs(l64['prio'] ), np.maximum(np.abs(sc.astype(f64)), 1.0)))
                else:
                    add_ulp('k_lch_loss priority (squared error)', i, out['prio'], l64['prio'], l32['prio'], top)
            dz = out['dzb'][i][:, :oc]
            add('k_lch_loss dz', i, dz, hc.st_dz(dl, p['lw'], feat, f64).reshape(B, oc, g.hw), hc.st_dz(dl, p['lw'], feat, f32).reshape(B, oc, g.hw))
            bpart = out['spart_bwd'][i][:, :oc]
            add('k_lch_loss backward partials', i, bpart, hc.st_bpart(dz, u, f64), hc.st_bpart(dz, u, f32))
            # k_lch_bnb on the kernel's partials and saved statistics
            n64 = hc.st_bnb(bpart, save[i, :oc, 0], save[i, :oc, 1], p['gamma'], float(B * g.hw), f64)
            n32 = hc.st_bnb(bpart, save[i, :oc, 0], save[i, :oc, 1], p['gamma'], float(B * g.hw), f32)
            for j, k in ((2, 'c1'), (3, 'c2'), (4, 'c3')):
                add(f'k_lch_bnb {k}', i, coef[i, :oc, j], n64[k], n32[k])
            c = [coef[i, :oc, j] for j in (2, 3, 4)]
            du_k[i] = (hc.st_du(dz, u, *c, f64), hc.st_du(dz, u, *c, f32))
            # k_lch_dw1 / k_lch_dlin: this step's partial gradients
            wp = hc.split_wpart(out['wpart'], g)[hd][t]
            add('k_lch_dw1 partial', i, wp['w1'], hc.st_dw1(du_k[i][0], F, f64), hc.st_dw1(du_k[i][1], F, f32))
            (lw64, lb64), (lw32, lb32) = hc.st_dlin(dl, feat, f64), hc.st_dlin(dl, feat, f32)
            add('k_lch_dlin dlw partial', i, wp['lw'], lw64, lw32)
            add('k_lch_dlin dlb partial', i, wp['lb'], lb64, lb32)
    for hd, (oc, *_r) in enumerate(H):
        o = 2 * sum(h[0] for h in H[:hd])
        add('k_lch_bn running_mean after K steps', hd, out['running_out'][o:o + oc], running64[hd][0], running[hd][0])
        add('k_lch_bn running_var after K steps', hd, out['running_out'][o + oc:o + 2 * oc], running64[hd][1], running[hd][1])
        # k_lch_bnb: dgamma / dbeta over the steps, from the kernel's partials
        per = [hc.st_bnb(out['spart_bwd'][3 * t + hd][:, :oc], save[3 * t + hd, :oc, 0], save[3 * t + hd, :oc, 1], case['heads'][hd]['gamma'], float(B * g.hw), f64) for t in range(g.K)]
        gr = hc.split_params(out['grads'], g)[hd]
        for k, key in (('gamma', 'dgamma'), ('beta', 'dbeta')):
            tot = np.sum([q[key] for q in per], 0)
            rows.append((f'k_lch_bnb {key}', hd, ulps(gr[k], tot, np.maximum(np.abs(tot), 2.0 ** -126)), 0.5, 1.0))  # (float64 sums rounded once: half an ulp, bar twice that)
    w1 = [case['heads'][hd]['w1'] for hd in range(3)]
    for t in range(g.K):
        r, p_, v = du_k[3 * t], du_k[3 * t + 1], du_k[3 * t + 2]
        add('k_lch_dx dF_pred', 3 * t + 1, out['dF_pred'][t], hc.st_dF([p_[0], v[0]], w1[1:], f64), hc.st_dF([p_[1], v[1]], w1[1:], f32))
        add('k_lch_dx dF_rew', 3 * t, out['dF_rew'][t], hc.st_dF([r[0]], w1[:1], f64), hc.st_dF([r[1]], w1[:1], f32))
    l64 = float(out['lpart'].astype(f64).sum()) / B
    rows.append(('k_lch_bnb loss', -1, ulps(out['loss'], [l64], [abs(l64)]), 0.5, 1.0))  # (a float64 sum of the kernel's terms, rounded once)
    return rows


def summarize(rows):
    """stage -> dict(kernel, chain, bar) of the group with the largest kernel / bar."""
    out = {}
    for stage, i, ek, ec, bar in rows:
        ratio = ek / bar if bar > 0 else (0.0 if ek == 0 else float('inf'))
        if stage not in out or ratio > out[stage]['ratio']:
            out[stage] = dict(kernel=ek, chain=ec, bar=bar, ratio=ratio, group=i)
    return out


_ROWS = {}


def rows_of(name, B):
    """stage_rows of the random case (name, B), with the bar the test holds each row to: its own (twice its chain) at a batch of 63 or more; below that the
    larger of its own and the largest of the same stage and head at the geometry's largest batch.  One or two images give the chain statistic one or two draws -- the ratio of two
    such draws says nothing -- while the stage's error per element does not grow as the batch shrinks (the batch sums get shorter); the small batches are
    there for the loops they enter."""
    if (name, B) not in _ROWS:
        case = hc.random_case(hc.GEOMS[name], B, hc.case_seed(name, B))
        rows = stage_rows(name, B, case, run(name, case))
        if B < 63:
            top = {}
            for stage, i, _, _, bar in rows_of(name, hc.BATCHES[name][-1]):
                top[(stage, i % 3)] = max(top.get((stage, i % 3), 0.0), bar)
            rows = [(stage, i, ek, ec, max(bar, top[(stage, i % 3)])) for stage, i, ek, ec, bar in rows]
        _ROWS[(name, B)] = rows
    return _ROWS[(name, B)]


def row_name(stage, i):
    if i < 0:
        return stage
    if stage.startswith(('k_lch_bn running', 'k_lch_bnb d')):
        return f'{stage}, {hc.HEAD_NAMES[i]} head'
    return f'{stage}, {hc.HEAD_NAMES[i % 3]} head, step {i // 3}'


@pytest.mark.parametrize('name,B', CASES)
def test_every_kernel_matches_float64_on_its_own_inputs(name, B):
    g = hc.GEOMS[name]
    rows = rows_of(name, B)
    for stage, v in sorted(summarize(rows).items()):
        print(f'  {name} B={B} {stage}: kernel {v["kernel"]:.3g}, chain {v["chain"]:.3g}, bar {v["bar"]:.3g} ({"ulps" if stage in ULP_STAGES else "rel rms"}), group {v["group"]}')
    bad = [f'{row_name(stage, i)}: {ek:.4g} against a bar of {bar:.4g} (float32 chain {ec:.4g})' for stage, i, ek, ec, bar in rows if not ek <= bar]
    assert not bad, f'{name} B={B}:\n' + '\n'.join(bad)
    case = hc.random_case(g, B, hc.case_seed(name, B))
    _wsum_is_step_order_sum(name, B, g, run(name, case, skip=('u', 'feat', 'dzb', 'dF_pred', 'dF_rew')))


# ---- c. end to end -----------------------------------------------------------------------------------------------------------------------------------------
# Every end-to-end output is a multiple of per-channel coefficients that were rounded to float32 once for the whole tensor -- a or b, then c1, c2 | c3 -- so
# it carries their relative errors (up to 2^-24 each, four on the longest path) coherently: no summation order reproduces them, no element count averages
# them, and the chain's own draw of them is one sample.  The chain's error is therefore taken as no smaller than four roundings.
E2E_FLOOR = 4 * 2.0 ** -24


def e2e_rows(name, case, out):
    g = hc.GEOMS[name]
    m64, m32 = hc.model(case, g), hc.model(case, g, dt=f32)
    rows = []

    def add(what, got, a, b):
        ec = rel_rms(b, a)
        rows.append((what, rel_rms(got, a), ec, 2.0 * max(ec, E2E_FLOOR)))

    add('loss', out['loss'], [m64['loss']], [np.float32(m32['loss'])])
    add('priorities', out['prio'], m64['prio'], m32['prio'])
    add('dF_pred', out['dF_pred'], m64['dF_pred'], m32['dF_pred'])
    add('dF_rew', out['dF_rew'], m64['dF_rew'], m32['dF_rew'])
    gr = hc.split_params(out['grads'], g)
    for hd, hn in enumerate(hc.HEAD_NAMES):
        oc = hc.heads(g)[hd][0]
        for k in ('w1', 'gamma', 'beta', 'lw', 'lb'):
            add(f'{hn} d{k}', gr[hd][k], m64['grads'][hd][k], m32['grads'][hd][k])
        o = 2 * sum(h[0] for h in hc.heads(g)[:hd])
        add(f'{hn} running_mean', out['running_out'][o:o + oc], m64['running'][hd][0], m32['running'][hd][0])
        add(f'{hn} running_var', out['running_out'][o + oc:o + 2 * oc], m64['running'][hd][1], m32['running'][hd][1])
    return rows


EDGES = [(n, B, v) for n, B in LAST for v in ('edge',)] + [(n, hc.BATCHES[n][-1], v) for n in ('board5', 'atari') for v in ('big_logits', 'gamma0', 'constant_plane')]


@pytest.mark.parametrize('name,B,which', EDGES)
def test_end_to_end_on_edge_data(name, B, which):
    g = hc.GEOMS[name]
    case = hc.edge_case(g, B, hc.case_seed(name, B))
    if which != 'edge':
        case = hc.variant(case, g, which)
    out = run(name, case)
    for k in ('loss', 'prio', 'dF_pred', 'dF_rew', 'grads', 'running_out'):
        assert np.isfinite(out[k]).all(), f'{name} B={B} {which}: {k} is not finite'
    assert (out['nbt_out'] == case['nbt'] + g.K).all()
    zero_w = case['w'] == 0
    if zero_w.any():  # a zero importance weight: the sample's loss gradient is exactly zero (its priority is not)
        assert (out['dlogit'][:, zero_w][np.isfinite(out['dlogit'][:, zero_w])] == 0).all() and (out['lpart'][:, zero_w] == 0).all()
    rows = e2e_rows(name, case, out)
    for what, ek, ec, bar in rows:
        print(f'  {name} B={B} {which} {what}: kernel {ek:.3g}, chain {ec:.3g}, bar {bar:.3g}')
    bad = [f'{what}: rms error {ek:.4g} of the model\'s rms against a bar of {bar:.4g} (float32 chain {ec:.4g})' for what, ek, ec, bar in rows if not ek <= bar]
    assert not bad, f'{name} B={B} {which}:\n' + '\n'.join(bad)


# ---- d. the handle, refusals -------------------------------------------------------------------------------------------------------------------------------
def test_the_hook_leaves_the_handle_untouched():
    """Weights, gradient and optimizer moments (one flat vector), running statistics and counters, and the tensors an update saved -- the heads' features,
    raw conv outputs of both shared towers, a hidden state -- are the same bytes after a call of the hook, and the next update is the same update."""
    from forced_masks import HipTensors
    name = 'board3'
    hl, g = _learner(name), hc.GEOMS[name]
    B = 5
    rs = np.random.RandomState(1)
    dev = torch.device('cuda', 0)
    ring = dict(state=torch.from_numpy(rs.uniform(0, 1, (B, 18)).astype(f32)).to(dev), action=torch.from_numpy(rs.randint(0, g.A, (B, g.K)).astype(np.int8)).to(dev),
                pi_prob=torch.from_numpy(rs.dirichlet(np.ones(g.A), size=(B, g.K)).astype(f32)).to(dev), value=torch.from_numpy(rs.uniform(-1, 1, (B, g.K)).astype(f32)).to(dev),
                reward=torch.from_numpy(rs.uniform(-1, 1, (B, g.K)).astype(f32)).to(dev))
    hl.grad(ring, None, None, B)
    ht = HipTensors(hl)

    def snap():
        torch.cuda.synchronize()
        saved = [ht.get('feat', 0, 0, (3 * g.K, B, 2 * g.hw)), ht.get('y', 1, 0, (B, g.P, g.hw)), ht.get('y', 1 + g.K, 0, (B, g.P, g.hw)), ht.get('s', 0, 0, (B, g.P, g.hw))]
        return [t.detach().cpu().numpy().tobytes() for t in (hl.flat, hl.running, hl.num_batches)] + [a.tobytes() for a in saved]

    before = snap()
    run(name, hc.random_case(g, 7, 5))
    assert snap() == before, 'mzl_debug_heads changed the learner\'s weights, gradient, optimizer moments, running statistics or saved tensors'
    hl.grad(ring, None, None, B)
    torch.cuda.synchronize()
    g1, l1, p1 = hl.grad_flat.detach().cpu().numpy().tobytes(), hl.loss.cpu().numpy().tobytes(), hl.priorities.cpu().numpy().tobytes()
    run(name, hc.random_case(g, 3, 6))
    hl.grad(ring, None, None, B)
    torch.cuda.synchronize()
    assert (hl.grad_flat.detach().cpu().numpy().tobytes(), hl.loss.cpu().numpy().tobytes(), hl.priorities.cpu().numpy().tobytes()) == (g1, l1, p1), \
        'an update after the hook differs from the same update before it'


def test_refusals_leave_the_handle_usable():
    from muzero_amd.hip_learner import LearnerError, MzlHeadsCall, load_library
    name = 'board3'
    hl, g = _learner(name), hc.GEOMS[name]
    good = hc.random_case(g, 4, 8)
    ref = run(name, good)
    big = hc.random_case(g, 131, 8)
    with pytest.raises(LearnerError, match='batch must be in'):
        run(name, big)
    empty = {k: (v[:0] if k in ('idx', 'w') else v) for k, v in good.items()}
    empty['F_pred'], empty['F_rew'] = good['F_pred'][:, :0], good['F_rew'][:, :0]
    with pytest.raises(LearnerError, match='batch must be in'):
        run(name, empty)
    with pytest.raises(LearnerError, match='idx out of'):
        run(name, dict(good, idx=np.array([0, 1, 2, good['value'].shape[0]], np.int64)))
    with pytest.raises(LearnerError, match='idx out of'):
        run(name, dict(good, idx=np.array([0, -1, 2, 1], np.int64)))
    lib = load_library()
    call = MzlHeadsCall()
    call.batch, call.rows = 4, 7
    assert lib.mzl_debug_heads(hl._h, C.byref(call)) != 0 and b'null argument' in lib.mzl_last_error()
    assert lib.mzl_debug_heads(hl._h, None) != 0 and b'null argument' in lib.mzl_last_error()
    # a learner without conv heads
    from helpers import build_mlp, mlp_case
    from muzero_amd.hip_learner import HipLearner
    dev = torch.device('cuda', 0)
    mlp = HipLearner(build_mlp(mlp_case('tiny')).to(dev), dev, 2, 8, lr=1e-3)
    try:
        with pytest.raises(LearnerError, match='needs a conv-net learner'):
            mlp.debug_heads(*[None] * 10)
    finally:
        mlp.close()
    again = run(name, good)
    for k in ref:
        assert ref[k].tobytes() == again[k].tobytes(), f'{k} differs after the refused calls'


def test_even_support_sizes_are_refused_at_create():
    """The expectation over the support is taken with unit spacing in every kernel (learner and planner); linspace(-half, half, S) has that spacing at odd
    S only (tests/test_heads_host.py), so an even S is refused where a handle is created."""
    from muzero_amd.hip_learner import HipLearner, LearnerError
    from muzero_amd.network import MuZeroAtariNet
    dev = torch.device('cuda', 0)
    for vs, rs_ in ((10, 11), (11, 10)):
        with pytest.raises(LearnerError, match='odd'):
            HipLearner(MuZeroAtariNet((4, 96, 96), 6, 1, 8, vs, rs_).to(dev), dev, 2, 4, lr=1e-3)
    from helpers import build_mlp
    from muzero_amd import planner as pl
    from test_gpu_api_errors import _cfg
    for vs, rs_ in ((6, 5), (7, 4)):
        net = build_mlp(('even', (3, 4), 3, 32, vs, rs_, 16, 14))
        with pytest.raises(LearnerError, match='odd'):
            HipLearner(net.to(dev), dev, 2, 4, lr=1e-3)
        with pytest.raises(pl.PlannerError, match='odd'):
            pl.Planner(_cfg(net, num_envs=1, num_simulations=3), 0)
    HipLearner(build_mlp(('odd', (3, 4), 3, 32, 7, 1, 16, 14)).to(dev), dev, 2, 4, lr=1e-3).close()  # (1 and odd sizes: as before)


if __name__ == '__main__':  # python tests/test_gpu_heads.py [out.json]: the accuracy table
    doc = {'statistic': 'per stage and geometry, the group (application) with the largest kernel / bar.  rel rms: rms(out - model64) / rms(model64) of one group\'s tensor; '
                        'ulps: the worst element\'s error in float32 ulps of its natural scale (stages through expf / logf / sqrtf / a division).  chain: the float32 '
                        'chain twin on the same inputs; bar: twice the chain (tensors under 64 elements: at least one correct rounding; batches under 63: the bar of the geometry\'s '
                        'largest batch); end to end: rel rms per tensor, the chain taken as at least four roundings', 'stages': {}, 'end_to_end': {}}
    for name, B in CASES:
        for stage, v in summarize(rows_of(name, B)).items():
            doc['stages'].setdefault(stage, {'unit': 'ulps' if stage in ULP_STAGES else 'rel rms'})[f'{name} B={B}'] = {k: float('%.4g' % v[k]) for k in ('chain', 'bar', 'kernel')}
    for name, B, which in EDGES:
        g = hc.GEOMS[name]
        case = hc.edge_case(g, B, hc.case_seed(name, B))
        if which != 'edge':
            case = hc.variant(case, g, which)
        doc['end_to_end'][f'{name} B={B} {which}'] = {what: {'chain': float('%.4g' % ec), 'bar': float('%.4g' % bar), 'kernel': float('%.4g' % ek)}
                                                      for what, ek, ec, bar in e2e_rows(name, case, run(name, case))}
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'heads', 'accuracy.json')
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    for h in _LEARNERS.values():
        h.close()
