"""The opt-in split-bf16 weight gradient of the board-net learner (mzl_set_wgrad_precision(MZL_WGRAD_BF16X3), HipLearner(wgrad_precision='bf16x3');
k_lc_wgrad_bf16x3 of muzero_amd/csrc/mz_learn_conv_split_wgrad.h) on a `board3` handle.

1. One launch through mzl_debug_wgrad on the integer classes of tests/wgrad_layer_cases.py plus this kernel's Locator positions
   (tests/wgrad_split_cases.py; tests/test_wgrad_split_host.py checks bounds, coverage and that every term is needed): the output EQUALS int64 -- at the
   update's choices, every SG the split budget allows, forced images per chunk, remap on and off, both action routes, accumulate, transforms,
   pairs, the K-steps launch.  Every case asserts what ran (build, SG, layout, ipw, act, remap) against what wgrad_split_cases.py wrote down.
2. Random data against float64: relative rms error at most BAR x a float32 chain's, whole tensor and per slice.  Bit-equal across runs, remap, pairing.
3. The whole gradient on six geometries at both conv_precision values: only the towers' conv weights differ from the wgrad_precision='f32' handle, and
   every tensor is within max(flat bar, 2 x the f32 learner's error).  4. The reference fixture.  5. Reproducibility.  6. Refusals.  7. Default = f32."""
import copy
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import conv_layer_cases as cc
import wgrad_layer_cases as wc
import wgrad_split_cases as sc
from helpers import build_conv, build_mlp, conv_case, mlp_case
from muzero_amd.replay import Transition
from test_gpu_conv_layer import BAR
from test_gpu_conv_learner import G, _batch, _net, _ring, _same_branch, same_branch_bar
from test_gpu_wgrad_layer import RANDOM_CASES, _random_reference, assert_equal, check_ran
from test_wgrad_layer_host import preload, steps_data, transform_cases

pytestmark = pytest.mark.gpu

_HANDLES = {}


def _hip(net, dev, max_batch, K=5, **kw):
    from muzero_amd.hip_learner import HipLearner

    kw.setdefault('lr', 1e-3)
    return HipLearner(net, dev, K, max_batch, **kw)


def _make(kind):
    dev = torch.device('cuda', 0)
    conv, wgrad = kind.split('/')
    return _hip(build_conv(conv_case('board3')).to(dev), dev, 4, conv_precision=conv, wgrad_precision=wgrad)


@pytest.fixture(scope='module')
def handle():
    """'<conv_precision>/<wgrad_precision>' -> a small board-net learner (the hook takes the handle's switches and CU count, nothing else)."""
    def get(kind='f32/bf16x3'):
        if kind not in _HANDLES:
            _HANDLES[kind] = _make(kind)
        return _HANDLES[kind]

    yield get
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def build_of(act):
    return 'k_lc_wgrad_bf16x3<ACT=1>' if act == 'kernel' else 'k_lc_wgrad_bf16x3<ACT=0>'


def strip(name):
    return re.sub(r' us=\S+', '', name)


# ------------------------------------------------------------------------------------------ 1a. plain launches
@pytest.mark.parametrize('rid', sc.PLAIN_IDS)
def test_integer_weight_gradient_is_exact(handle, rid):
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    e = sc.expect_plain(rid)
    hl = handle()
    n = 0
    for cls, i, dz, x, kw, ref in sc.int_cases(run['shape'], e['sg'], e['ipw']):
        out, name = hl.debug_wgrad(dz, x, **kw, **run['over'])
        what = f'{rid} class {cls} draw {i}'
        check_ran(name, what, mode='plain', SG=e['sg'], layout=e['layout'], ipw=e['ipw'], act=e['act'], precision='f32', build=build_of(e['act']), P4=e['P'],
                  nsteps=e['nsteps'], **({} if e['remap'] is None else dict(remap=e['remap'])))
        assert_equal(out, ref, what, name, locate=(B, cr, board, board) if cls.startswith('locator') and not A else None)
        n += 1
    print(f'{rid}: {n} launches EQUAL, {name}')


@pytest.mark.parametrize('key,layout,sg', sc.SG_RUNS, ids=[f'{k}-sg{s}-{"cols" if l == 1 else "rows"}' for k, l, s in sc.SG_RUNS])
def test_every_sg_the_split_budget_allows_is_exact(handle, key, layout, sg):
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    ipw = sc.images_per_chunk(B, sg, cout, cr)
    P, ns = sc.planes(board, board, sg, layout == 2)[:2]
    for cls, i, dz, x, kw, ref in sc.int_cases(key, sg, ipw, layout == 2):
        out, name = handle().debug_wgrad(dz, x, sg=sg, layout=layout, **kw)
        what = f'{key} sg {sg} layout {layout} class {cls} draw {i}'
        check_ran(name, what, SG=sg, layout='single' if sg == 1 else ('cols' if layout == 1 else 'rows'), ipw=ipw, P4=P, nsteps=ns, build=build_of('none'))
        assert_equal(out, ref, what, name, locate=(B, cr, board, board) if cls.startswith('locator') else None)


@pytest.mark.parametrize('key,layout,sg', sc.SG_REFUSED)
def test_an_sg_over_the_split_budget_is_refused_not_launched(handle, key, layout, sg):
    from muzero_amd.hip_learner import LearnerError

    board, cr, cin, A, cout, B = wc.SHAPES[key]
    dz, x = wc.int_draws(key, 'dense')[0]
    with pytest.raises(LearnerError, match='mzl_debug_wgrad: SG override'):
        handle().debug_wgrad(dz, x, sg=sg, layout=layout)
    if key.startswith('b15'):  # (two 15 x 15 images per round: the float32 planes do not hold them either)
        with pytest.raises(LearnerError, match='mzl_debug_wgrad: SG override'):
            handle('f32/f32').debug_wgrad(dz, x, sg=sg, layout=layout)


# ------------------------------------------------------------------------------------------ 1b. accumulate, 1c. transforms
@pytest.mark.parametrize('rid', wc.ACCUMULATE_RUNS)
def test_accumulate_adds_to_a_nonzero_preload(handle, rid):
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    e = sc.expect_plain(rid)
    pre = preload(cout, cin)
    for cls, i, dz, x, kw, ref in sc.int_cases(run['shape'], e['sg'], e['ipw']):
        if cls == 'locator8' and i > 0:
            continue
        out, name = handle().debug_wgrad(dz, x, preload=pre, accumulate=True, **kw, **run['over'])
        check_ran(name, rid, act=e['act'], SG=e['sg'], ipw=e['ipw'], build=build_of(e['act']))
        assert_equal(out, ref + pre.astype(np.int64), f'{rid} accumulate class {cls} draw {i}', name)
        out, name = handle().debug_wgrad(dz, x, preload=pre, accumulate=False, **kw, **run['over'])
        assert_equal(out, ref, f'{rid} overwrite class {cls} draw {i}', name)


@pytest.mark.parametrize('rid', wc.TRANSFORM_RUNS)
def test_staging_transforms_are_exact_on_the_wide_class(handle, rid):
    run = wc.PLAIN_RUNS[rid]
    e = sc.expect_plain(rid)
    for cls, i, dz, x, kw in transform_cases(rid):
        ref = wc.wgrad64(dz, x, dtype=np.int64, **kw)
        assert wc.int_bound(dz, x, **kw)[0] < 2 ** 24
        out, name = handle().debug_wgrad(dz, x, **kw, **run['over'])
        check_ran(name, rid, SG=e['sg'], ipw=e['ipw'], build=build_of('none'))
        assert_equal(out, ref, f'{rid} {"dcoef + xcoef (IN_BNRELU)" if "xcoef" in kw else "dcoef, identity x"}', name)


# ------------------------------------------------------------------------------------------ 1d. pairs, 1e. steps
@pytest.mark.parametrize('pid', list(wc.PAIR_RUNS))
def test_paired_launch_is_exact_for_both_layers(handle, pid):
    first, second, over, _ = wc.PAIR_RUNS[pid]
    sg, ipw, remap = sc.expect_pair(pid)
    a, b = sc.int_cases(first, sg, ipw), sc.int_cases(second, sg, ipw)
    for k in range(max(len(a), len(b))):
        (ca, ia, dza, xa, _, refa), (cb, ib, dzb, xb, _, refb) = a[k % len(a)], b[(k + 1) % len(b)]
        (outa, outb), name = handle().debug_wgrad(dza, xa, mode='pair', second=dict(dz=dzb, x=xb), **over)
        check_ran(name, pid, mode='pair', SG=sg, ipw=ipw, remap=remap, build=build_of('none'))
        assert_equal(outa, refa, f'{pid} first layer {first} class {ca} draw {ia}', name)
        assert_equal(outb, refb, f'{pid} second layer {second} class {cb} draw {ib}', name)


@pytest.mark.parametrize('sid', list(wc.STEP_RUNS))
def test_steps_launch_is_exact(handle, sid):
    key, nsrc, over, _ = wc.STEP_RUNS[sid]
    sg, ipw, cps = sc.expect_steps(sid)
    for cls, i, dz, x in steps_data(key, nsrc):
        ref = wc.wgrad64(dz.reshape((-1,) + dz.shape[2:]), x.reshape((-1,) + x.shape[2:]), dtype=np.int64)
        out, name = handle().debug_wgrad(dz, x, mode='steps', **over)
        check_ran(name, sid, mode='steps', SG=sg, ipw=ipw, cps=cps, nsrc=nsrc, chunks=nsrc * cps, build=build_of('none'))
        assert_equal(out, ref, f'{sid} class {cls} draw {i}', name)


# ------------------------------------------------------------------------------------------ 2. random data against float64
SPLIT_RANDOM = ('b9_40to48', 'b15_64to80')


def measure_random(hl, cid):
    """(name, {slice: (E kernel, E chain32)}) of one random case (the data, reference and chain of tests/test_gpu_wgrad_layer.py)."""
    board, cin, cout, B, ipw = RANDOM_CASES[cid]
    dz, x, ref, e_chain = _random_reference(board, board, cin, cout, B, False)
    out, name = hl.debug_wgrad(dz, x, ipw=ipw)
    return name, {s: (cc.rel_rms(out, ref, ax), e_chain[s]) for s, ax in wc.SLICES.items()}


@pytest.mark.parametrize('cid', SPLIT_RANDOM)
def test_random_weight_gradient_matches_float64_within_twice_a_float32_chain(handle, cid):
    """Measured on an MI355X (profiles/split_wgrad/accuracy.json): see README."""
    name, st = measure_random(handle(), cid)
    check_ran(name, cid, build=build_of('none'))
    print(f'{cid}: {name}')
    for s, (e, ec) in st.items():
        r = np.asarray(e / ec)
        print(f'  {s}: E kernel {np.max(e):.3g} (max), E chain32 {np.max(ec):.3g} (max), ratio max {r.max():.3f} median {np.median(r):.3f} over {r.size} slices')
    for s, (e, ec) in st.items():
        assert np.all(e <= BAR * ec), f'{cid} {s}: E = {np.max(e / ec):.3f} x chain32 (bar {BAR}), {name}'


def test_one_summation_order_across_runs_remap_and_pairing(handle):
    hl = handle()
    key = 'b6_128to128_n8'
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    rs = np.random.RandomState(11)
    x, dz = cc.random_values(rs, (B, cr, board, board), (B, cout, board, board))
    x2, dz2 = cc.random_values(rs, (B, cr, board, board), (B, cout, board, board))
    o_on, n_on = hl.debug_wgrad(dz, x, remap=1)
    o_on2, _ = hl.debug_wgrad(dz, x, remap=1)
    o_off, n_off = hl.debug_wgrad(dz, x, remap=2)
    check_ran(n_on, 'remap on', remap=1, build=build_of('none'))
    check_ran(n_off, 'remap off', remap=0, build=build_of('none'))
    assert o_on.tobytes() == o_on2.tobytes() and o_on.tobytes() == o_off.tobytes()
    ipw = int(re.search(r'ipw=(\d+)', n_on).group(1))
    (pa, pb), n_pair = hl.debug_wgrad(dz, x, mode='pair', second=dict(dz=dz2, x=x2), ipw=ipw)
    o2, _ = hl.debug_wgrad(dz2, x2, ipw=ipw)
    check_ran(n_pair, 'pair', mode='pair', ipw=ipw, build=build_of('none'))
    assert pa.tobytes() == o_on.tobytes() and pb.tobytes() == o2.tobytes()
    assert not np.array_equal(o_on, handle('f32/f32').debug_wgrad(dz, x)[0])  # (another arithmetic, not the float32 kernel's bits)


# ------------------------------------------------------------------------------------------ 3. the whole gradient
WHOLE = [(3, 16, 2, 9, 4, False), (5, 8, 1, 5, 7, False), (6, 128, 1, 2, 17, True), (9, 32, 3, 9, 64, True), (15, 16, 1, 9, 3, False), (15, 32, 2, 9, 10, True)]


def _is_tower_conv(name, hl):
    return hl.views[name].dim() == 4 and hl.views[name].shape[-1] == 3


@pytest.mark.parametrize('conv', ('f32', 'bf16x3'))
@pytest.mark.parametrize('board,planes,blocks,chan,B,int8_state', WHOLE, ids=[f'b{g[0]}-p{g[1]}-r{g[2]}-n{g[4]}' for g in WHOLE])
def test_whole_gradient_differs_in_tower_conv_weights_only_and_stays_float32_grade(board, planes, blocks, chan, B, int8_state, conv):
    from test_gpu_conv_learner import GEOMETRIES

    assert (board, planes, blocks, chan, B, int8_state) in GEOMETRIES
    dev = torch.device('cuda', 0)
    net, A = _net(board, planes, blocks, chan, 100 + board, dev)
    net.train()
    rs = np.random.RandomState(board * 7 + B)
    tr = _batch(rs, B, (chan, board, board), A, K=5, int8_state=int8_state)
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    net32 = copy.deepcopy(net)
    h32 = _hip(net32, dev, B, conv_precision=conv, wgrad_precision='f32')
    loss32, prio32 = h32.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    e32 = _same_branch(h32, net32, tr, w, B, 5, dev)[0]
    hl = _hip(net, dev, B, conv_precision=conv, wgrad_precision='bf16x3')
    loss, prio = hl.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    assert hl.wgrad_precision == 1 and h32.wgrad_precision == 0
    # 3.1 only the towers' conv weights move
    assert torch.equal(loss, loss32) and torch.equal(prio, prio32)
    moved = 0
    sparse = sc.sparse_route(planes, planes + A)
    for k in hl.views:
        a, b = hl.grad_views[k], h32.grad_views[k]
        if not _is_tower_conv(k, hl):
            assert torch.equal(a, b), k
        else:
            moved += int(not torch.equal(a, b))
            if sparse and a.shape[1] == planes + A:  # the dynamics net's first conv: its action-plane rows are the float32 gather's
                assert torch.equal(a[:, planes:], b[:, planes:]), k
    assert moved > 0
    # 3.2 float32-grade: every tensor within max(flat bar, 2 x the f32 learner's error)
    errs, err_t32, _, _, flipped = _same_branch(hl, net, tr, w, B, 5, dev)
    _, _, flat_bar = same_branch_bar(errs, err_t32)
    worst = max(errs, key=lambda k: errs[k] / max(flat_bar, 2.0 * e32[k]))
    bar = max(flat_bar, 2.0 * e32[worst])
    print(f'b{board}-p{planes}-r{blocks}-n{B} conv {conv}: {moved} tower conv weights differ; worst tensor {worst} {errs[worst]:.2e} bar {bar:.2e} (wgrad f32: {e32[worst]:.2e})')
    assert errs[worst] <= bar, (worst, errs[worst], bar, e32[worst], flipped)
    h32.close()
    hl.close()


# ------------------------------------------------------------------------------------------ 4. the reference fixture
@pytest.mark.parametrize('conv', ('f32', 'bf16x3'))
def test_loss_gradients_and_three_updates_match_the_reference(conv):
    """tests/test_gpu_split_learner.py test_split_loss_gradients_and_three_updates_match_the_reference with the split weight gradient."""
    pre = 'learn_conv_board3'
    dev = torch.device('cuda', 0)
    net = build_conv(conv_case('board3')).to(dev)
    net.train()
    hl = _hip(net, dev, 16, lr=1e-3, milestones=[2], gamma=0.1, max_grad_norm=10.0, conv_precision=conv, wgrad_precision='bf16x3')
    tr = Transition(*[G[f'{pre}_{f}'] for f in Transition._fields])
    B = tr.state.shape[0]
    ring = _ring(tr, dev)
    w = torch.from_numpy(G[f'{pre}_weights']).to(dev)
    losses = []
    for step in range(3):
        loss, prio = hl.grad(ring, None, w, B)
        if step == 0:
            np.testing.assert_allclose(prio.cpu().numpy(), G[f'{pre}_prio'], rtol=1e-3, atol=1e-3)
            for pn in hl.views:
                ref = G[f'{pre}_grad_{pn}']
                np.testing.assert_allclose(hl.grad_views[pn].cpu().numpy(), ref, rtol=2e-3, atol=2e-3 * float(np.abs(ref).max()) + 1e-7, err_msg=pn)
        hl.apply(clip=(step == 1))
        losses.append(float(loss))
    np.testing.assert_allclose(losses, G[f'{pre}_losses'], rtol=1e-4)
    sd = net.state_dict()
    for pn in sd:
        ref = G[f'{pre}_final_{pn}']
        np.testing.assert_allclose(sd[pn].cpu().numpy(), ref, rtol=2e-3, atol=2e-5 + 1e-4 * float(np.abs(ref).max()), err_msg=pn)
    assert abs(hl.current_lr() - 1e-4) < 1e-12 and hl.steps == 3
    hl.close()


# ------------------------------------------------------------------------------------------ 5. reproducibility
def _one_update(net, tr, w, B, dev, env=None, **kw):
    if env:
        os.environ[env] = '1'
    try:
        hl = _hip(copy.deepcopy(net), dev, B, **kw)
    finally:
        if env:
            del os.environ[env]
    loss, prio = hl.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    g, loss, prio = hl.grad_flat.clone(), loss.clone(), prio.clone()
    hl.apply()
    out = (g, loss, prio, hl.params.clone(), hl.running.clone())
    hl.close()
    return out


WHAT = ('gradient', 'loss', 'priorities', 'weights', 'running statistics')


@pytest.mark.parametrize('board,planes,blocks', [(15, 16, 1), (9, 32, 3)])
def test_update_is_bit_reproducible_across_runs_and_pairings(board, planes, blocks):
    dev = torch.device('cuda', 0)
    net, A = _net(board, planes, blocks, 4, 60 + board, dev)
    rs = np.random.RandomState(board)
    B = 6
    tr = _batch(rs, B, (4, board, board), A)
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    first = _one_update(net, tr, w, B, dev, wgrad_precision='bf16x3')
    for env in (None, 'MZLC_NO_PAIR', 'MZLC_NO_SIDE'):
        other = _one_update(net, tr, w, B, dev, env=env, wgrad_precision='bf16x3')
        for a, b, what in zip(first, other, WHAT):
            assert torch.equal(a, b), (env, what)
    f32 = _one_update(net, tr, w, B, dev)
    assert not torch.equal(first[0], f32[0]) and torch.equal(first[1], f32[1])  # (another arithmetic in the gradient; the same forward pass)


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(handle):
    from muzero_amd import hip_learner as hlm
    from muzero_amd.network import MuZeroAtariNet

    dev = torch.device('cuda', 0)
    lib = hlm.load_library()
    with pytest.raises(hlm.LearnerError, match='wgrad_precision.*MZL_NET_MLP|MZL_NET_MLP.*wgrad_precision'):
        _hip(build_mlp(mlp_case('tiny')).to(dev), dev, 4, wgrad_precision='bf16x3')
    with pytest.raises(hlm.LearnerError, match='wgrad_precision.*MZL_NET_ATARI|MZL_NET_ATARI.*wgrad_precision'):
        _hip(MuZeroAtariNet((4, 96, 96), 6, 1, 8, 11, 11).to(dev), dev, 2, wgrad_precision='bf16x3')
    with pytest.raises(ValueError, match='wgrad_precision'):
        _hip(build_conv(conv_case('board3')).to(dev), dev, 4, wgrad_precision=2)
    # the ABI itself on a bound float32 handle: an unknown value is MZL_E_INVALID, a known one after mzl_bind MZL_E_STATE; the handle stays float32
    hl = handle('f32/f32')
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    _, before = hl.debug_wgrad(z(2, 8, 3, 3), z(2, 4, 3, 3))
    assert before.startswith('f32 k_lc_wgrad<ACT=0,RING=0>')
    assert lib.mzl_set_wgrad_precision(hl._h, 2) == -1 and 'wgrad_precision' in lib.mzl_last_error().decode()
    assert lib.mzl_set_wgrad_precision(hl._h, -1) == -1 and 'wgrad_precision' in lib.mzl_last_error().decode()
    assert lib.mzl_set_wgrad_precision(hl._h, 1) == -3 and 'mzl_bind' in lib.mzl_last_error().decode()
    assert lib.mzl_set_wgrad_precision(hl._h, 0) == -3
    assert lib.mzl_set_wgrad_precision(None, 1) == -1
    _, after = hl.debug_wgrad(z(2, 8, 3, 3), z(2, 4, 3, 3))
    assert strip(before) == strip(after)
    # and the same on the split handle: it stays split
    hs = handle()
    assert lib.mzl_set_wgrad_precision(hs._h, 0) == -3
    _, n = hs.debug_wgrad(z(2, 8, 3, 3), z(2, 4, 3, 3))
    assert n.startswith('f32 k_lc_wgrad_bf16x3<ACT=0>'), n
    # the hook's first token stays the handle's conv_precision
    _, n = handle('bf16x3/bf16x3').debug_wgrad(z(2, 8, 3, 3), z(2, 4, 3, 3))
    assert n.startswith('bf16x3 k_lc_wgrad_bf16x3<ACT=0>'), n
    with pytest.raises(hlm.LearnerError, match='mzl_debug_wgrad.*Atari handle'):
        hs.debug_wgrad(z(1, 8, 14, 14), z(1, 4, 14, 14), mode='ring')


# ------------------------------------------------------------------------------------------ 7. the default is float32
def test_default_and_explicit_f32_are_the_same_bits_and_the_same_kernel(handle):
    dev = torch.device('cuda', 0)
    net, A = _net(9, 32, 2, 4, 91, dev)
    rs = np.random.RandomState(9)
    B = 7
    tr = _batch(rs, B, (4, 9, 9), A)
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    a = _one_update(net, tr, w, B, dev)
    for v in ('f32', 0):
        b = _one_update(net, tr, w, B, dev, wgrad_precision=v)
        for x, y, what in zip(a, b, WHAT):
            assert torch.equal(x, y), (v, what)
    board, cin, cout, Bn, _ = RANDOM_CASES['b9_40to48']
    dz, x, _, _ = _random_reference(board, board, cin, cout, Bn, False)
    never = _hip(build_conv(conv_case('board3')).to(dev), dev, 4)
    (o0, n0), (o1, n1) = never.debug_wgrad(dz, x), handle('f32/f32').debug_wgrad(dz, x)
    assert never.wgrad_precision == 0 and handle('f32/f32').wgrad_precision == 0
    assert n0.startswith('f32 k_lc_wgrad<ACT=0,RING=0>') and strip(n0) == strip(n1) and o0.tobytes() == o1.tobytes()
    never.close()


if __name__ == '__main__':  # python tests/test_gpu_wgrad_split.py <out.json>: the ratios of the random cases, as the test measures them
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    result = {'statistic': 'rms(out - wgrad64) / rms(wgrad64); ratio = kernel / chain32 (a sequential float32 sum over images and positions)', 'bar': BAR, 'cases': {}}
    h = _make('f32/bf16x3')
    for cid in SPLIT_RANDOM:
        name, st = measure_random(h, cid)
        entry = {'ran': strip(name), 'chain32': float('%.4g' % float(st['whole'][1])), 'kernel': float('%.4g' % float(st['whole'][0])),
                 'ratio': round(float(st['whole'][0] / st['whole'][1]), 4)}
        for s in ('cout', 'cin', 'tap'):
            r = np.asarray(st[s][0] / st[s][1])
            entry[f'{s}_slices'] = {'n': int(r.size), 'ratio_min': round(float(r.min()), 4), 'ratio_median': round(float(np.median(r)), 4), 'ratio_max': round(float(r.max()), 4)}
        result['cases'][cid] = entry
    h.close()
    with open(sys.argv[1], 'w') as f:
        json.dump(result, f, indent=1)
        f.write('\n')
    print(json.dumps(result, indent=1))
