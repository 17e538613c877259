"""Reloading planner weights from device memory (mz_planner_bind_param_device / mz_planner_refresh_params, muzero_amd/csrc/mz_pack.h).

The yardstick is the host path: a planner H loaded with `load_state_dict` (mz_planner_set_param + mz_planner_commit_params).  A planner D
that never sees a host tensor -- only bound to the same values in GPU memory and refreshed -- must hold the same BYTES in every packed
buffer (mz_debug_read_packed: a wrong weight in a padding slot multiplies a zero activation and never shows in an output), and compute
the same outputs.  Equality everywhere: the refresh repeats the commit's float32 operations in the commit's order."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import build_conv, build_mlp, conv_case, mlp_case, seeded_state_dict

pytestmark = pytest.mark.gpu

BOARD = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0))
SEARCH = {'cartpole': {}, 'lunar': {}, 'tiny': {}, 'tiny_mse': {}, 'odd': {}, 'tictactoe': BOARD, 'board3': BOARD, 'board5': BOARD, 'board9': BOARD,
          'atari_s': {}, 'atari_m': {}}
MLP = ('cartpole', 'tictactoe', 'lunar', 'tiny', 'tiny_mse', 'odd')


def _net(name):
    return build_mlp(mlp_case(name)) if name in MLP else build_conv(conv_case(name))


def _planner(net, name, num_envs=8, precision='f32', sims=16, seed=3):
    from muzero_amd import planner as pl

    return pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=num_envs, seed=seed, num_simulations=sims, conv_precision=precision,
                                        **SEARCH.get(name, BOARD)), 0)


def _gpu(sd):
    return {k: v.to('cuda:0').contiguous() for k, v in sd.items() if not k.endswith('num_batches_tracked')}


def _pair(name, precision='f32', net=None, **kw):
    """(net, H loaded through the host, D bound and refreshed on the GPU, the tensors D is bound to)."""
    net = net if net is not None else _net(name)
    H, D = _planner(net, name, precision=precision, **kw), _planner(net, name, precision=precision, **kw)
    H.load_state_dict(net.state_dict())
    w = _gpu(net.state_dict())
    D.bind_device_weights(w)
    D.refresh_weights()
    return net, H, D, w


def _assert_same_packed(H, D):
    h, d = H.read_packed(), D.read_packed()
    assert len(h) > 0 and [x[0] for x in h] == [x[0] for x in d]
    for (label, _, hb), (_, _, db) in zip(h, d):
        assert len(hb) == len(db), label
        if hb != db:
            a, b = np.frombuffer(hb, np.uint8), np.frombuffer(db, np.uint8)
            bad = np.flatnonzero(a != b)
            raise AssertionError(f'{label}: {bad.size} of {a.size} bytes differ, first at byte {bad[0]}')
    return [x[0] for x in h]


PACKED = [(n, 'f32') for n in MLP] + [(n, 'f32') for n in ('board3', 'board5', 'board9', 'atari_s', 'atari_m')] + [('board3', 'bf16x3'), ('board9', 'bf16x3')]


@pytest.mark.parametrize('name,precision', PACKED, ids=[f'{n}-{p}' for n, p in PACKED])
def test_packed_bytes_equal_the_host_commit(name, precision):
    _, H, D, _ = _pair(name, precision)
    labels = _assert_same_packed(H, D)
    if name in ('cartpole', 'tictactoe', 'lunar'):
        assert 'fast_stream' in labels and 'bias_all' in labels
    if name == 'board3':
        split = precision == 'bf16x3'  # (split mode runs one launch per conv: no fused-tower tables, mz_convnet.h)
        assert 'dyn_sp_w' in labels and 'dyn_act_w' in labels and 'dyn_sp_terms' in labels
        assert ('dyn_res.tw' in labels) == (not split) and ('rep_conv.w3' in labels) == split
    stats = D.pack_stats()
    assert stats['launches'] == (2 if precision == 'bf16x3' else 1) and stats['bytes_written'] > 0


def test_packed_bytes_under_the_generic_kernel_switch():
    """MZ_FORCE_GENERIC is read when a handle is created: a fresh child process."""
    env = dict(os.environ, MZ_FORCE_GENERIC='1')
    r = subprocess.run([sys.executable, os.path.abspath(__file__), 'cartpole'], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'packed-equal' in r.stdout, r.stdout + r.stderr


def test_packed_bytes_of_a_full_width_board_net():
    """15 x 15, 128 planes, one block: the tower-table and dynamics-conv sizes of the C5 net (bytes only, no search)."""
    from muzero_amd import network

    net = network.MuZeroBoardGameNet((9, 15, 15), 226, 1, 128)
    net.load_state_dict(seeded_state_dict(net, 31))
    net.eval()
    _, H, D, _ = _pair('board15', net=net, num_envs=1, sims=1)
    labels = _assert_same_packed(H, D)
    assert 'pred_res.tw' in labels and 'dyn_sp_terms' in labels


def _outputs(p, net, name, rs):
    shape = tuple(net.planner_spec()['input_shape'])
    B, A = 8, p.A
    obs = rs.uniform(0, 1, (B,) + shape).astype(np.float32)
    h0, pi0, v0 = p.initial_inference(obs)
    act = rs.randint(0, A, B).astype(np.int32)
    h1, r1, pi1, v1 = p.recurrent_inference(h0, act)
    noise = rs.dirichlet(np.ones(A), size=B)
    board = bool(SEARCH[name])
    s = p.search(obs, np.ones((B, A), np.uint8), 1, 2 if board else 1, 1.0, noise=noise, u_tie=rs.uniform(0, 1, (B, p.max_ties)), u_final=rs.uniform(0, 1, B))
    return [h0, pi0, v0, h1, r1, pi1, v1, s['action'], s['pi'], s['root_value'], s['visits']]


OUTPUTS = [('cartpole', 'f32'), ('tictactoe', 'f32'), ('board3', 'f32'), ('board3', 'bf16x3'), ('atari_s', 'f32')]


@pytest.mark.parametrize('name,precision', OUTPUTS, ids=[f'{n}-{p}' for n, p in OUTPUTS])
def test_outputs_equal_the_host_path(name, precision):
    net, H, D, _ = _pair(name, precision)
    a, b = _outputs(H, net, name, np.random.RandomState(5)), _outputs(D, net, name, np.random.RandomState(5))
    for i, (x, y) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(x, y, err_msg=f'output {i}')
    assert a[7].shape == (8,) and np.isfinite(a[9]).all()


@pytest.mark.parametrize('name', ['board3', 'cartpole'])
def test_refresh_in_place_after_the_tensors_were_overwritten_on_a_side_stream(name):
    net, _, D, w = _pair(name)
    before = [(label, addr) for label, addr, _ in D.read_packed()]
    sd2 = seeded_state_dict(net, 900)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for k, t in w.items():
            t.copy_(sd2[k].to('cuda:0', non_blocking=True))
    D.refresh_weights(side)
    H2 = _planner(net, name)
    H2.load_state_dict(sd2)
    _assert_same_packed(H2, D)
    assert [(label, addr) for label, addr, _ in D.read_packed()] == before  # written in place
    obs = np.random.RandomState(2).uniform(0, 1, (4,) + tuple(net.planner_spec()['input_shape'])).astype(np.float32)
    for x, y in zip(H2.initial_inference(obs), D.initial_inference(obs)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('name', ['tictactoe', 'board9'])
def test_reload_in_the_middle_of_self_play(name):
    """Two moves, new weights, two moves: the same records whether the reload went through the host or through a refresh (same seed)."""
    from muzero_amd import planner as pl

    net = _net(name)
    sd1, sd2 = net.state_dict(), seeded_state_dict(net, 901)
    env = pl.ENV_TICTACTOE if name == 'tictactoe' else pl.ENV_GOMOKU
    sims = 16 if name == 'tictactoe' else 4
    H, D = _planner(net, name, sims=sims, seed=9), _planner(net, name, sims=sims, seed=9)
    H.load_state_dict(sd1)
    w = _gpu(sd1)
    D.bind_device_weights(w)
    D.refresh_weights()
    for p in (H, D):
        p.selfplay_reset(env)
        p.selfplay_step(-1.0, 2)
    H.load_state_dict(sd2)
    with torch.no_grad():
        for k, t in w.items():
            t.copy_(sd2[k].to('cuda:0'))
    D.refresh_weights()
    for p in (H, D):
        p.selfplay_step(-1.0, 2)
    a, b = H.selfplay_read(4), D.selfplay_read(4)
    assert set(a) == set(b) == {'obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done'}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    _assert_same_packed(H, D)


def test_host_commit_after_a_bind_and_refresh_after_it():
    """board3: the host commit reallocates every buffer; the next refresh must follow them."""
    net, _, D, w = _pair('board3')
    sd2, sd3 = seeded_state_dict(net, 902), seeded_state_dict(net, 903)
    D.load_state_dict(sd2)
    H = _planner(net, 'board3')
    H.load_state_dict(sd2)
    _assert_same_packed(H, D)
    with torch.no_grad():
        for k, t in w.items():
            t.copy_(sd3[k].to('cuda:0'))
    D.refresh_weights()
    H.load_state_dict(sd3)
    _assert_same_packed(H, D)
    obs = np.random.RandomState(3).uniform(0, 1, (4, 9, 3, 3)).astype(np.float32)
    for x, y in zip(H.initial_inference(obs), D.initial_inference(obs)):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize('name,key', [('board3', 'dynamics_net.conv_block.1.running_var'), ('tictactoe', 'prediction_net.value_net.2.bias')])
def test_refresh_with_a_tensor_unbound_names_it(name, key):
    from muzero_amd import planner as pl

    net = _net(name)
    D = _planner(net, name)
    w = _gpu(net.state_dict())
    del w[key]
    D.bind_device_weights(w)
    with pytest.raises(pl.PlannerError, match=r'error -3: .*' + key.rsplit('.', 1)[0].replace('.', r'\.')):
        D.refresh_weights()
    with pytest.raises(pl.PlannerError, match='-3'):  # and the handle is not usable
        D.initial_inference(np.zeros((1,) + tuple(net.planner_spec()['input_shape']), np.float32))


@pytest.mark.parametrize('name,key', [('board3', 'represent_net.conv_block.0.weight'), ('tictactoe', 'dynamics_net.transition_net.0.weight')])
def test_wrong_shape_is_invalid(name, key):
    from muzero_amd import planner as pl

    net = _net(name)
    D = _planner(net, name)
    w = _gpu(net.state_dict())
    w[key] = w[key].transpose(0, 1).contiguous()
    with pytest.raises(pl.PlannerError, match='error -1: .*' + key.replace('.', r'\.')):
        D.bind_device_weights(w)
        D.refresh_weights()


def test_host_pointer_is_invalid():
    net = _net('tiny')
    D = _planner(net, 'tiny')
    a = np.zeros((32, 12), np.float32)
    shape = (C.c_int64 * 2)(32, 12)
    rc = D.lib.mz_planner_bind_param_device(D.h, b'represent_net.net.0.weight', a.ctypes.data_as(C.c_void_p), shape, 2)
    assert rc == -1 and b'represent_net.net.0.weight' in D.lib.mz_last_error()
    pinned = torch.zeros(32, 12).pin_memory()
    rc = D.lib.mz_planner_bind_param_device(D.h, b'represent_net.net.0.weight', C.c_void_p(pinned.data_ptr()), shape, 2)
    assert rc == -1
    t = torch.zeros(7, dtype=torch.int64, device='cuda:0').view(torch.float32)[:2]
    rc = D.lib.mz_planner_bind_param_device(D.h, b'x.num_batches_tracked', C.c_void_p(t.data_ptr()), (C.c_int64 * 1)(2), 1)
    assert rc == -1


def _random_batch(rs, B, obs_shape, A, K=5):
    from muzero_amd.replay import Transition

    return Transition(rs.randint(0, 2, (B,) + obs_shape).astype(np.int8), rs.randint(0, A, (B, K)).astype(np.int8),
                      rs.dirichlet(np.ones(A), size=(B, K)).astype(np.float32), rs.uniform(-1, 1, (B, K)).astype(np.float32),
                      rs.uniform(-1, 1, (B, K)).astype(np.float32))


@pytest.mark.parametrize('name', ['tictactoe', 'board3'])
def test_learner_hand_off(name):
    """Two updates of the HIP learner, then its master weights (and, conv nets, the running statistics its kernels wrote) straight into
    the planner: the bytes a host reload of `net.state_dict()` packs."""
    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    net = _net(name).to(dev)
    net.train()
    B = 16
    hl = HipLearner(net, dev, 5, B, lr=1e-2)
    D = _planner(net, name)
    D.bind_device_weights(hl.planner_weights())
    D.refresh_weights()
    first = D.read_packed()
    rs = np.random.RandomState(8)
    shape = tuple(net.planner_spec()['input_shape'])
    for _ in range(2):
        tr = _random_batch(rs, B, shape, net.planner_spec()['num_actions'])
        ring = dict(state=torch.from_numpy(tr.state).to(dev).reshape(B, -1).contiguous(), action=torch.from_numpy(tr.action).to(dev),
                    pi_prob=torch.from_numpy(tr.pi_prob).to(dev), value=torch.from_numpy(tr.value).to(dev), reward=torch.from_numpy(tr.reward).to(dev))
        hl.grad(ring, None, torch.ones(B, device=dev), B)
        hl.apply()
    D.refresh_weights()
    net.eval()
    H = _planner(net, name)
    H.load_state_dict(net.state_dict())
    _assert_same_packed(H, D)
    assert [b for _, _, b in first] != [b for _, _, b in D.read_packed()]  # the updates changed the weights
    assert D.reload(hl.planner_weights()) == 'device' and D.reload(net.state_dict()) == 'device'  # the module's tensors are the same memory
    _assert_same_packed(H, D)


if __name__ == '__main__':  # child of test_packed_bytes_under_the_generic_kernel_switch
    _, H_, D_, _ = _pair(sys.argv[1])
    _assert_same_packed(H_, D_)
    assert 'MZ_FORCE_GENERIC=1' in D_.describe()
    print('packed-equal')
