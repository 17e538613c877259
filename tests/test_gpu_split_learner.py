"""The opt-in split-bf16 convs of the board-net learner (mzl_config.conv_precision = MZL_CONV_BF16X3, muzero_amd/csrc/mz_learn_conv_split.h):
the towers' forward convs and data gradients on v_mfma_f32_16x16x32_bf16, every float32 operand the exact sum of three bf16 values.

1. One conv through mzl_debug_conv (the learner's own packers, tiling chooser and dispatcher), both directions, both precisions, on integer data
   whose every partial sum is an exact float32 (tests/conv_layer_cases.py classes W, X, M; tests/test_split_learner_host.py checks the bounds on
   these shapes): the output EQUALS the int64 conv.  A lost term stream, k slot, tap flip or transposition meets a value that needs it.
2. One conv on seeded random data against float64: relative rms error over the whole output, per channel and per pixel at most BAR = 2 x that
   of a plain float32 chain -- the bar, statistics and slice size of tests/test_gpu_conv_layer.py, for both precisions.
3. The whole gradient over the geometries of tests/test_gpu_conv_learner.py, float64 autograd on the pass's own branch: every tensor within
   max(the f32 path's bar, 2 x the f32 HIP learner's error for that tensor on the same batch).
4.-7. The reference fixture, other unroll lengths, bit-reproducibility across builds and launch pairings, six updates against the autograd learner.
8. Refusals.  9. The default path and conv_precision='f32' are the same bits."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import conv_layer_cases as cc
from helpers import build_conv, build_mlp, conv_case, mlp_case
from muzero_amd import learner
from muzero_amd.replay import Transition
from test_gpu_conv_layer import BAR, MIN_SLICE
from test_gpu_conv_learner import GEOMETRIES, G, _batch, _f64_reference, _net, _ring, _same_branch, same_branch_bar
from test_split_learner_host import INT_SHAPES, flip_transpose, int_case

pytestmark = pytest.mark.gpu
PRECISIONS = ('f32', 'bf16x3')


def _hip(net, dev, max_batch, K=5, **kw):
    from muzero_amd.hip_learner import HipLearner

    kw.setdefault('lr', 1e-3)
    return HipLearner(net, dev, K, max_batch, **kw)


_HANDLES = {}


@pytest.fixture(scope='module')
def handle():
    """precision -> a small board-net learner of that conv_precision (the hook takes its precision and its switches, nothing else)."""
    def get(precision):
        if precision not in _HANDLES:
            dev = torch.device('cuda', 0)
            _HANDLES[precision] = _hip(build_conv(conv_case('board3')).to(dev), dev, 4, conv_precision=precision)
        return _HANDLES[precision]

    yield get
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


# ------------------------------------------------------------------------------------------ 1. one conv, exact integers
INT_RUNS = [(s, d) for s in INT_SHAPES for d in (0, 1) if not (d == 1 and INT_SHAPES[s][3])]


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('shape,direction', INT_RUNS)
def test_integer_conv_is_exact(handle, shape, direction, precision):
    board, cr, cin, A, cout, B = INT_SHAPES[shape]
    hl = handle(precision)
    launches = 0
    for cls in cc.INT_CLASSES:
        x, action, xf, draws = int_case(cls, shape, direction)
        for i, (wt, _) in enumerate(draws):
            out, name = hl.debug_conv(direction, wt, x, action=action, num_actions=A, cin=cin)
            assert precision in name and ('bf16x3' in name) == (precision == 'bf16x3'), name
            if board == 15:
                assert 'SIDE=15' in name, name
            wref = flip_transpose(wt) if direction else wt
            ref = cc.int_reference(xf, wref, np.zeros(wref.shape[0], np.float32)).astype(np.float32)
            bad = np.argwhere(out != ref)
            assert len(bad) == 0, (f'{precision} class {cls} {shape} direction {direction} draw {i} (reduction channels {cc._live(wref).tolist()}, {name}): '
                                   f'{len(bad)} outputs differ, first at (image, channel, y, x) = {bad[0].tolist()}: {out[tuple(bad[0])]} != {ref[tuple(bad[0])]}')
            launches += 1
    print(f'{shape} direction {direction} {precision}: {launches} launches, {name}')


# ------------------------------------------------------------------------------------------ 2. one conv, random data
# id: (board, cin, cout, batch at least); the batch is raised until every per-channel and per-pixel slice has MIN_SLICE values, as in test_gpu_conv_layer
RANDOM_SHAPES = {'b9_40to48': (9, 40, 48, 4), 'b15_64to80': (15, 64, 80, 2)}


@functools.lru_cache(maxsize=None)
def _random_reference(shape, direction):
    """(input, the hook's weight, float64 reference, the chain's statistics): computed once, shared by both precisions, never written to."""
    board, cin, cout, b0 = RANDOM_SHAPES[shape]
    k_in, c_out = (cin, cout) if direction == 0 else (cout, cin)
    B = max(b0, -(-MIN_SLICE // c_out), -(-MIN_SLICE // (board * board)))
    d = cc.random_layer(2000 + 2 * sorted(RANDOM_SHAPES).index(shape) + direction, B, k_in, k_in, c_out, board, board)
    ref = cc.conv64(d['x'], d['w'])
    c32 = cc.chain32(d['x'], d['w'])
    assert min(B * board * board, B * c_out) >= MIN_SLICE
    e_chain = {s: cc.rel_rms(c32, ref, ax) for s, ax in cc.SLICES.items()}
    w_hook = d['w'] if direction == 0 else flip_transpose(d['w'])  # [cout, cin, 3, 3] of the forward layer either way
    for a in (d['x'], w_hook, ref):
        a.setflags(write=False)
    return d['x'], w_hook, ref, e_chain


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('direction', (0, 1))
@pytest.mark.parametrize('shape', list(RANDOM_SHAPES))
def test_random_conv_matches_float64_within_twice_a_float32_chain(handle, shape, direction, precision):
    x, w_hook, ref, e_chain = _random_reference(shape, direction)
    out, name = handle(precision).debug_conv(direction, w_hook, x)
    print(f'{shape} direction {direction} {precision}: {name}')
    assert precision in name
    for s, ax in cc.SLICES.items():
        e, ec = cc.rel_rms(out, ref, ax), e_chain[s]
        r = np.asarray(e / ec)
        print(f'  {s}: E kernel {np.max(e):.3g} (max), E chain32 {np.max(ec):.3g} (max), ratio max {r.max():.3f} median {np.median(r):.3f} over {r.size} slices')
        assert np.all(e <= BAR * ec), f'{shape} direction {direction} {precision} {s}: E = {r.max():.3f} x chain32 (bar {BAR})'


# ------------------------------------------------------------------------------------------ 3. the whole gradient
def split_vs_f32_errors(board, planes, blocks, chan, B, int8_state, dev, K=5):
    """Both learners on one batch: (split learner, its errors per tensor, PyTorch-float32's errors on its branch, the f32 HIP learner's errors per
    tensor, loss, float64 loss on the branch, decisions float64 would have taken differently, batch pieces).  Every error is against float64
    autograd told what THAT pass decided (tests/forced_masks.py): the f32 learner's on its own decisions, which are the split learner's
    wherever no pre-activation sits within rounding of zero."""
    net, A = _net(board, planes, blocks, chan, 100 + board, dev)
    net.train()
    rs = np.random.RandomState(board * 7 + B)
    tr = _batch(rs, B, (chan, board, board), A, K=K, int8_state=int8_state)
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    net32 = copy.deepcopy(net)
    h32 = _hip(net32, dev, B, K=K)
    h32.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    e32 = _same_branch(h32, net32, tr, w, B, K, dev)[0]
    h32.close()
    hl = _hip(net, dev, B, K=K, conv_precision='bf16x3')
    loss, prio = hl.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    errs, err_t32, loss_d, prio_d, flipped = _same_branch(hl, net, tr, w, B, K, dev)
    return dict(hl=hl, net=net, tr=tr, w=w, errs=errs, err_t32=err_t32, e32=e32, loss=float(loss), prio=prio, loss_d=loss_d, flipped=flipped)


def worst_against_bar(r):
    """(tensor, error, bar, True if only the second term of the bar admits it) of the tensor furthest over (or closest to) its bar."""
    _, _, flat_bar = same_branch_bar(r['errs'], r['err_t32'])
    worst = None
    for k, e in r['errs'].items():
        bar = max(flat_bar, 2.0 * r['e32'][k])
        if worst is None or e / bar > worst[1] / worst[2]:
            worst = (k, e, bar, e > flat_bar)
    return worst


@pytest.mark.parametrize('board,planes,blocks,chan,B,int8_state', GEOMETRIES, ids=[f'b{g[0]}-p{g[1]}-r{g[2]}-n{g[4]}' for g in GEOMETRIES])
def test_split_gradient_matches_float64_autograd(board, planes, blocks, chan, B, int8_state):
    dev = torch.device('cuda', 0)
    r = split_vs_f32_errors(board, planes, blocks, chan, B, int8_state, dev)
    net, tr, w = r['net'], r['tr'], r['w']
    # loss, priorities, running statistics: plain float64 autograd from the module's start values (they do not depend on the branch to first order)
    net0, _ = _net(board, planes, blocks, chan, 100 + board, dev)
    net0.train()
    loss_p, prio_p, _, sd0, closest = _f64_reference(net0, tr._replace(state=tr.state.astype(np.float64)), w, dev)
    assert abs(r['loss'] - loss_p) <= 1e-4 * max(1.0, abs(loss_p))
    np.testing.assert_allclose(r['prio'].cpu().numpy(), prio_p.cpu().numpy(), rtol=1e-3, atol=1e-4)
    assert abs(r['loss'] - r['loss_d']) <= 2e-6 * max(1.0, abs(r['loss_d']))
    k, e, bar, second = worst_against_bar(r)
    print(f'b{board}-p{planes}-r{blocks}-n{B}: worst tensor {k} {e:.2e} bar {bar:.2e} (f32 HIP learner {r["e32"][k]:.2e})' + (' -- passes through the second term only' if second and e <= bar else ''))
    assert e <= bar, (k, e, bar, 'f32 HIP learner:', r['e32'][k], 'decisions float64 would have taken differently:', r['flipped'], 'closest', closest)
    # running statistics and num_batches_tracked: one train-mode step per application
    sd = net.state_dict()
    for kk, v in sd0.items():
        if 'running' in kk:
            assert float((v - sd[kk].double()).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max())), kk
        if 'num_batches_tracked' in kk:
            assert int(v) == int(sd[kk]), kk
    r['hl'].close()


# ------------------------------------------------------------------------------------------ 4. the reference fixture
def test_split_loss_gradients_and_three_updates_match_the_reference():
    """tests/test_gpu_conv_learner.py's recipe on `learn_conv_board3` (three updates, clip on the second, an LR milestone) at its own tolerances."""
    pre = 'learn_conv_board3'
    dev = torch.device('cuda', 0)
    net = build_conv(conv_case('board3')).to(dev)
    net.train()
    hl = _hip(net, dev, 16, lr=1e-3, milestones=[2], gamma=0.1, max_grad_norm=10.0, conv_precision='bf16x3')
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


# ------------------------------------------------------------------------------------------ 5. other unroll lengths
@pytest.mark.parametrize('K', [1, 8])
def test_split_other_unroll_lengths(K):
    dev = torch.device('cuda', 0)
    net, A = _net(5, 16, 1, 3, 300 + K, dev)
    net.train()
    rs = np.random.RandomState(K)
    B = 5
    tr = _batch(rs, B, (3, 5, 5), A, K=K)
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    loss_p, _, _, sd_d, closest = _f64_reference(net, tr._replace(state=tr.state.astype(np.float64)), w, dev)
    hl = _hip(net, dev, B, K=K, conv_precision='bf16x3')
    loss, prio = hl.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    assert abs(float(loss) - loss_p) <= 1e-4 * max(1.0, abs(loss_p))
    errs, err32, _, _, flipped = _same_branch(hl, net, tr, w, B, K, dev)
    k, e, bar = same_branch_bar(errs, err32)
    assert e <= bar, (k, e, bar, K, flipped)
    sd = net.state_dict()
    for k, v in sd_d.items():
        if 'num_batches_tracked' in k:
            assert int(v) == int(sd[k]), k


# ------------------------------------------------------------------------------------------ 6. reproducibility
def _one_update(net, tr, w, B, dev, env=None, **kw):
    """(gradient, loss, priorities, weights after one update) of a fresh learner built under the environment switch `env`."""
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


@pytest.mark.parametrize('board,planes,blocks', [(15, 16, 1), (9, 32, 3)])
def test_split_update_is_bit_reproducible_across_builds_and_pairings(board, planes, blocks):
    dev = torch.device('cuda', 0)
    net, A = _net(board, planes, blocks, 4, 60 + board, dev)
    rs = np.random.RandomState(board)
    B = 6
    tr = _batch(rs, B, (4, board, board), A)
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    first = _one_update(net, tr, w, B, dev, conv_precision='bf16x3')
    for env in (None, 'MZLC_NO_SIDE', 'MZLC_NO_PAIR'):
        other = _one_update(net, tr, w, B, dev, env=env, conv_precision='bf16x3')
        for a, b, what in zip(first, other, ('gradient', 'loss', 'priorities', 'weights', 'running statistics')):
            assert torch.equal(a, b), (env, what)
    f32 = _one_update(net, tr, w, B, dev)
    assert not torch.equal(first[0], f32[0])  # (the switch really selects another arithmetic)


# ------------------------------------------------------------------------------------------ 7. six updates
def test_split_six_updates_follow_the_autograd_learner():
    """tests/test_gpu_conv_learner.py test_six_updates_follow_the_autograd_learner, the HIP learner in bf16x3, at that test's bars."""
    dev = torch.device('cuda', 0)
    net_b, A = _net(5, 8, 1, 5, 77, dev)
    net_a = copy.deepcopy(net_b).double()
    net_a.train()
    net_b.train()
    opt = torch.optim.Adam(net_a.parameters(), lr=2e-3, weight_decay=1e-4)
    sch = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[3], gamma=0.1)
    B = 12
    hl = _hip(net_b, dev, B, lr=2e-3, weight_decay=1e-4, milestones=[3], gamma=0.1, clip_grad=True, max_grad_norm=5.0, conv_precision='bf16x3')
    rs = np.random.RandomState(5)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    for step in range(6):
        tr = _batch(rs, B, (5, 5, 5), A)
        w = rs.uniform(0.3, 1.0, B).astype(np.float32)
        opt.zero_grad()
        la, pa = learner.loss_tensors(net_a, t(tr.state, torch.float64), t(tr.action, torch.int64), t(tr.value, torch.float64), t(tr.reward, torch.float64),
                                      t(tr.pi_prob, torch.float64), t(w, torch.float64))
        la.backward()
        torch.nn.utils.clip_grad_norm_(net_a.parameters(), 5.0)
        opt.step()
        sch.step()
        lb, pb = hl.step_transitions(tr, w)
        la = la.detach()
        assert abs(float(la) - float(lb)) <= 1e-3 * max(1.0, abs(float(la))), (step, float(la), float(lb))
        np.testing.assert_allclose(pb.cpu().numpy(), pa.detach().cpu().numpy(), rtol=5e-3, atol=5e-3)
        assert abs(sch.get_last_lr()[0] - hl.current_lr()) < 1e-12
    for (n, x), (_, y) in zip(net_a.state_dict().items(), net_b.state_dict().items()):
        d = (x.double() - y.double()).abs()
        sc = max(1.0, float(x.double().abs().max()))
        assert float(d.mean()) < 2e-4 * sc and float(d.max()) < 1.4e-2 * sc, (n, float(d.mean()), float(d.max()))


# ------------------------------------------------------------------------------------------ 8. refusals
def test_split_refusals():
    from muzero_amd import hip_learner as hlm
    from muzero_amd.network import MuZeroAtariNet

    dev = torch.device('cuda', 0)
    with pytest.raises(hlm.LearnerError, match='conv_precision.*MZL_NET_MLP|MZL_NET_MLP.*conv_precision'):
        _hip(build_mlp(mlp_case('tiny')).to(dev), dev, 4, conv_precision='bf16x3')
    with pytest.raises(hlm.LearnerError, match='conv_precision.*MZL_NET_ATARI|MZL_NET_ATARI.*conv_precision'):
        _hip(MuZeroAtariNet((4, 96, 96), 6, 1, 8, 11, 11).to(dev), dev, 2, conv_precision='bf16x3')
    with pytest.raises(ValueError, match='conv_precision'):
        _hip(build_conv(conv_case('board3')).to(dev), dev, 4, conv_precision=2)
    # the ABI itself: a config whose field holds 2
    lib = hlm.load_library()
    cfg = hlm.MzlConfig(9 * 3 * 3, 10, 16, 1, 1, 1, 5, 4, 1, hlm.NET_BOARD, 9, 3, 3, 2, 2)
    h = C.c_void_p()
    assert lib.mzl_create(C.byref(cfg), 0, C.byref(h)) == -1 and not h
    msg = lib.mzl_last_error().decode()
    assert 'conv_precision' in msg and 'MZL_NET_BOARD' in msg, msg
    # the hook validates its arguments
    hl = _hip(build_conv(conv_case('board3')).to(dev), dev, 4, conv_precision='bf16x3')
    ok_w, ok_x = np.zeros((4, 4, 3, 3), np.float32), np.zeros((1, 4, 3, 3), np.float32)
    hl.debug_conv(0, ok_w, ok_x)
    for direction, wt, x, kw in ((2, ok_w, ok_x, {}), (0, ok_w, np.zeros((1, 4, 16, 16), np.float32), {}), (0, np.zeros((4, 6, 3, 3), np.float32), ok_x, {}),
                                 (1, ok_w, np.zeros((1, 5, 3, 3), np.float32), {}),
                                 (0, np.zeros((4, 6, 3, 3), np.float32), ok_x, dict(action=np.array([3], np.int32), num_actions=3))):
        with pytest.raises(hlm.LearnerError, match='mzl_debug_conv'):
            hl.debug_conv(direction, wt, x, **kw)
    hl.close()


# ------------------------------------------------------------------------------------------ 9. float32 unmoved
def test_default_and_explicit_f32_are_the_same_bits(handle):
    dev = torch.device('cuda', 0)
    net, A = _net(9, 32, 2, 4, 91, dev)
    rs = np.random.RandomState(9)
    B = 7
    tr = _batch(rs, B, (4, 9, 9), A)
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    a = _one_update(net, tr, w, B, dev)
    b = _one_update(net, tr, w, B, dev, conv_precision='f32')
    for x, y, what in zip(a, b, ('gradient', 'loss', 'priorities', 'weights', 'running statistics')):
        assert torch.equal(x, y), what
    d = cc.random_layer(4, 2, 8, 8, 8, 5, 5)
    for hl in (_hip(copy.deepcopy(net), dev, B), handle('f32')):
        assert hl.conv_precision == 0
        out, name = hl.debug_conv(0, d['w'], d['x'])
        assert name.startswith('f32 k_lc_conv ') and 'bf16x3' not in name, name
        np.testing.assert_allclose(out, cc.conv64(d['x'], d['w']), rtol=1e-5, atol=1e-5)
