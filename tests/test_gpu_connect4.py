"""The device Connect Four env (mz_selfplay_reset_connect4, csrc/mz_connect4.h) on an MI355X, held to `games.ConnectFourEnv` byte for byte:
the scripted games of connect4_cases.py through the debug step, several side by side with auto-resets; searched self-play in lock-step
with a host-stepped planner fed by host envs, records and replay rings (float32 and int8) identical; n moves in one call; the searches
against the oracle on the non-square boards; one HipLearner gradient from the rings; the refusals."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import connect4_cases as cc
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu

REC = ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')
BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
CFG = types.SimpleNamespace(is_board_game=True, acc_seq_length=9999, unroll_steps=5, td_steps=0, discount=1.0)
# The lock-step runs: shape -> (envs, moves, planner seed).  The seeds were picked on the GPU (the first of 1..8 that meets the
# conditions test_lock_step_self_play asserts from the host envs' own records).
LOCK = {'S': (9, 40, 1), 'F': (6, 24, 1)}
SIMS = 8


def _net(shape, planes=8, blocks=1, seed=31):
    from muzero_amd.network import MuZeroBoardGameNet

    rows, cols, _ = cc.SHAPES[shape]
    net = MuZeroBoardGameNet((9, rows, cols), cols + 1, blocks, planes)
    net.load_state_dict(seeded_state_dict(net, seed + rows))
    net.eval()
    return net


def _planner(net, B, sims=SIMS, seed=5, capture=False, **kw):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, num_simulations=sims, seed=seed, **dict(BOARD_KW, **kw)), 0)
    p.load_state_dict(net.state_dict())
    if capture:
        p.lib.mz_debug_capture_rng.argtypes = [C.c_void_p, C.c_int32]
        p.lib.mz_debug_read_rng.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        assert p.lib.mz_debug_capture_rng(p.h, 1) == 0
    return p


def _host_env(shape):
    from muzero_amd.games import ConnectFourEnv

    return ConnectFourEnv(*cc.SHAPES[shape])


@pytest.mark.parametrize('shape', ['S', 'T', 'F'])
def test_scripted_games_on_the_kernel(shape):
    """Every scripted game of the shape as one env of one planner, played through the debug step beside a host env.  An env plays its
    game again and again (a game that does not end by itself is ended by a resignation), so the envs finish at different plies and reset
    while their neighbours play on.  After every ply the record, the mask, the counters and the next observation equal the host's."""
    rows, cols, win = cc.SHAPES[shape]
    games = cc.cases(shape)
    scripts = [c['moves'] + ([] if c['done'] else [cols]) for c in games]
    B, plies = len(games), rows * cols + 8
    p = _planner(_net(shape), B)
    p.selfplay_reset_connect4(win)
    envs = [_host_env(shape) for _ in range(B)]
    at = [0] * B
    episodes = steps_done = 0
    ends = []
    assert np.array_equal(p.debug_connect4_mask(), np.ones((B, cols + 1), np.uint8))
    for ply in range(plies):
        obs = np.stack([e.observation() for e in envs]).astype(np.float32).reshape(B, -1)
        players = np.array([e.current_player for e in envs], np.int32)
        acts = np.array([scripts[i][at[i]] for i in range(B)], np.int32)
        p.debug_connect4_step(acts)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for i, e in enumerate(envs):
            _, rew[i], d, _ = e.step(int(acts[i]))
            at[i] += 1
            if d:
                assert at[i] == len(scripts[i]), (games[i]['name'], ply)  # the game ended where its case says, not before
                assert np.array_equal(e.board, cc.board_array(games[i]['board']))
                steps_done += e.steps
                e.reset()
                at[i], done[i] = 0, 1
            else:
                assert at[i] < len(scripts[i]), (games[i]['name'], ply)
        episodes += int(done.sum())
        ends.append(done)
        rec = p.selfplay_read(1)
        assert rec['obs'][0].tobytes() == obs.tobytes(), ply
        assert np.array_equal(rec['action'][0], acts) and np.array_equal(rec['player'][0], players), ply
        assert rec['reward'][0].tobytes() == rew.tobytes(), (ply, rec['reward'][0], rew)
        assert np.array_equal(rec['done'][0], done), (ply, rec['done'][0], done)
        assert np.array_equal(rec['pi'][0], np.eye(cols + 1)[acts]) and not rec['root_value'][0].any()
        assert np.array_equal(p.debug_connect4_mask(), np.stack([e.actions_mask for e in envs]).astype(np.uint8)), ply
        c = p.selfplay_counters()
        assert (c['env_steps'], c['simulations'], c['episodes'], c['episode_steps']) == (B * (ply + 1), 0, episodes, steps_done), (ply, c)
    ends = np.stack(ends)
    assert episodes >= 2 * B and len({int(np.flatnonzero(ends[:, i])[0]) for i in range(B)}) > 4  # the envs finish at different plies
    # the state after the last ply (fresh boards where a game has just ended) is what the next record shows
    obs = np.stack([e.observation() for e in envs]).astype(np.float32).reshape(B, -1)
    p.debug_connect4_step(np.array([int(np.flatnonzero(e.actions_mask)[0]) for e in envs], np.int32))
    assert p.selfplay_read(1)['obs'][0].tobytes() == obs.tobytes()
    p.close()


def _replay(cap, state):
    from muzero_amd.replay import PrioritizedReplay

    kw = dict(state_format='int8') if state == 'int8' else {}
    return PrioritizedReplay(cap, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw)


def _snap(rp, origin):
    torch.cuda.synchronize()
    return ({k: v.cpu().numpy().copy() for k, v in rp._ring.items()}, rp._attached[0].cpu().numpy().copy(), origin.cpu().numpy().copy())


CAP = 96


@functools.lru_cache(maxsize=None)
def lock_step(shape, seed=None):
    """A device Connect Four planner and a host-stepped planner fed by host ConnectFourEnv objects, for each replay state format (none,
    float32, int8), same seed, stepped in lock-step with the board temperature schedule.  Everything the tests below read."""
    B, M, picked = LOCK[shape]
    seed = picked if seed is None else seed
    rows, cols, win = cc.SHAPES[shape]
    net = _net(shape)
    side = {}
    for where in ('host', 'dev'):
        for state in (None, 'f32', 'int8'):
            p = _planner(net, B, seed=seed)
            rp = origin = None
            if state is not None:
                rp = _replay(CAP, state)
                origin = p.attach_replay(rp, CFG, obs_shape=(9, rows, cols), with_origin=True)
            if where == 'dev':
                p.selfplay_reset_connect4(win)
            else:
                p.selfplay_reset_external(frame_shape=(9, rows, cols), temp_switch_steps=6, max_episode_steps=rows * cols)
            side[(where, state)] = (p, rp, origin)
    envs = [_host_env(shape) for _ in range(B)]
    obs = [e.reset() for e in envs]
    base = ('host', None)
    equal, actions_equal, dones, counts = [], [], [], []
    lengths, column_filled, mid_game = [], False, False
    for m in range(M):
        acts = {}
        mask = np.stack([e.actions_mask for e in envs])
        cur, opp = [e.current_player for e in envs], [e.opponent_player for e in envs]
        for k, (p, _, _) in side.items():
            if k[0] == 'host':
                acts[k] = p.external_act(np.stack(obs), mask, cur, opp, -1.0)
            else:
                p.selfplay_step(-1.0, 1)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for i, e in enumerate(envs):
            obs[i], rew[i], d, _ = e.step(int(acts[base][i]))
            column_filled |= not e.actions_mask[:cols].all()
            if d:
                lengths.append(e.steps)
                obs[i] = e.reset()
            done[i] = d
        mid_game |= bool(done.any()) and any(e.steps > 0 for e in envs)
        for k, (p, _, _) in side.items():
            if k[0] == 'host':
                p.external_commit(rew, done)
            p.synchronize()
        recs = {k: p.selfplay_read(1) for k, (p, _, _) in side.items()}
        actions_equal.append(all(np.array_equal(recs[k]['action'][0], acts[base]) for k in side))
        equal.append({k: all(recs[base][f].tobytes() == recs[k][f].tobytes() for f in REC) for k in side})
        dones.append(done)
        counts.append({k: rp.num_added for k, (_, rp, _) in side.items() if rp is not None})
    n_last = min(M, 16)
    last = {k: p.selfplay_read(n_last) for k, (p, _, _) in side.items()}
    counters = {k: p.selfplay_counters() for k, (p, _, _) in side.items()}
    snap = {k: _snap(rp, origin) for k, (_, rp, origin) in side.items() if rp is not None}
    for p, _, _ in side.values():
        p.close()
    return types.SimpleNamespace(B=B, M=M, side=list(side), equal=equal, actions_equal=actions_equal, dones=np.stack(dones), counts=counts, last=last,
                                 counters=counters, snap=snap, base=base, lengths=lengths, column_filled=column_filled, mid_game=mid_game,
                                 net=net, shape=shape)


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    lock_step.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('shape', ['S', 'F'])
def test_lock_step_self_play(shape):
    r = lock_step(shape)
    assert all(r.actions_equal), [m for m, ok in enumerate(r.actions_equal) if not ok]
    for k in r.side:
        assert all(eq[k] for eq in r.equal), (k, [m for m, eq in enumerate(r.equal) if not eq[k]])
        for f in REC:
            assert r.last[k][f].tobytes() == r.last[r.base][f].tobytes(), (k, f)
        assert r.counters[k] == r.counters[r.base], k
    c = r.counters[r.base]
    assert c['env_steps'] == r.M * r.B and c['simulations'] == r.M * r.B * SIMS and c['episodes'] == r.dones.sum() == len(r.lengths)
    assert c['episode_steps'] == sum(r.lengths)
    # the run shows something: episodes ended and reset, not all at once, and (on S) a column filled up
    assert len(r.lengths) >= 3, r.lengths
    assert r.mid_game
    if shape == 'S':
        assert r.column_filled


@pytest.mark.parametrize('shape', ['S', 'F'])
def test_replay_rings_are_byte_identical(shape):
    r = lock_step(shape)
    assert all(len(set(c.values())) == 1 for c in r.counts), r.counts  # num_added after every move, all sides and formats
    n = r.counts[-1][('dev', 'f32')]
    assert n == sum(r.lengths) > 0  # a board game's items arrive when its episode ends
    for state, dt in (('f32', np.float32), ('int8', np.int8)):
        ring0, prio0, org0 = r.snap[('host', state)]
        ring1, prio1, org1 = r.snap[('dev', state)]
        assert ring0['state'].dtype == dt
        for f in ring0:
            assert ring0[f].dtype == ring1[f].dtype and ring0[f].tobytes() == ring1[f].tobytes(), (state, f)
        assert prio0.tobytes() == prio1.tobytes() and org0.tobytes() == org1.tobytes(), state
    f32, i8 = r.snap[('dev', 'f32')][0], r.snap[('dev', 'int8')][0]
    k = min(n, CAP)
    assert np.array_equal(f32['state'].reshape(CAP, -1)[:k], i8['state'].reshape(CAP, -1)[:k].astype(np.float32))
    for f in ('action', 'pi_prob', 'value', 'reward'):
        assert f32[f].tobytes() == i8[f].tobytes(), f
    assert set(np.unique(f32['value'][:k])) <= {-1.0, 0.0, 1.0}  # Monte-Carlo returns


@pytest.mark.parametrize('shape', ['S', 'F'])
def test_n_moves_in_one_call(shape):
    """n moves in one mz_selfplay_step equal n calls of one, and both are the lock-step run's device side."""
    B, M, seed = LOCK[shape]
    _, _, win = cc.SHAPES[shape]
    r = lock_step(shape)
    out = []
    for chunks in ([1] * M, [7, 1, M - 8]):
        p = _planner(r.net, B, seed=seed)
        rp = _replay(CAP, 'int8')
        origin = p.attach_replay(rp, CFG, obs_shape=(9,) + cc.SHAPES[shape][:2], with_origin=True)
        p.selfplay_reset_connect4(win)
        for n in chunks:
            p.selfplay_step(-1.0, n)
        p.synchronize()
        out.append((rp.num_added, _snap(rp, origin), p.selfplay_read(min(M, 16)), p.selfplay_counters()))
        p.close()
    ref = (r.counts[-1][('dev', 'int8')], r.snap[('dev', 'int8')], r.last[('dev', 'int8')], r.counters[('dev', 'int8')])
    for other, what in ((out[1], 'chunked'), (ref, 'lock-step')):
        a = out[0]
        assert a[0] == other[0] and a[3] == other[3], what
        assert all(a[1][0][f].tobytes() == other[1][0][f].tobytes() for f in a[1][0]), what
        assert a[1][1].tobytes() == other[1][1].tobytes() and a[1][2].tobytes() == other[1][2].tobytes(), what
        assert all(a[2][f].tobytes() == other[2][f].tobytes() for f in REC), what


@pytest.mark.parametrize('shape', ['S', 'F'])
def test_self_play_search_equals_the_oracle(oracle, shape):
    """3 moves of 4 envs: the recorded observation, the host env's mask and players and the captured Philox draws through
    oracle.uct_search_batch give the device move's policy (the visit distribution: temperature 1 in the first moves), root value and
    action.  The first oracle check of a non-square board net inside a game."""
    from test_oracle_nets import _oracle_net

    rows, cols, win = cc.SHAPES[shape]
    B, A = 4, cols + 1
    net = _net(shape)
    p = _planner(net, B, seed=77, capture=True)
    p.selfplay_reset_connect4(win)
    onet = _oracle_net(oracle, net, 'conv')
    cfg = oracle.make_config(A, SIMS, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    envs = [_host_env(shape) for _ in range(B)]
    for m in range(3):
        p.selfplay_step(-1.0, 1)
        noise, utie, ufin = np.empty((B, A), np.float64), np.empty((B, p.max_ties), np.float64), np.empty(B, np.float64)
        assert p.lib.mz_debug_read_rng(p.h, noise.ctypes.data_as(C.c_void_p), utie.ctypes.data_as(C.c_void_p), ufin.ctypes.data_as(C.c_void_p)) == 0
        rec = p.selfplay_read(1)
        obs = np.stack([e.observation() for e in envs]).astype(np.float32)
        assert rec['obs'][0].tobytes() == obs.tobytes()
        mask = np.stack([e.actions_mask for e in envs]).astype(np.uint8)
        cur = np.array([e.current_player for e in envs], np.int32)
        o = oracle.uct_search_batch(cfg, onet, obs, mask, cur, 3 - cur, 1.0, False, noise=noise, u_tie=utie, u_final=ufin)
        assert not np.isnan(o['pi']).any()
        np.testing.assert_array_equal(rec['pi'][0] * SIMS, o['visits'], err_msg=f'move {m}: visit counts')
        np.testing.assert_array_equal(rec['pi'][0], o['pi'], err_msg=f'move {m}: policy')
        np.testing.assert_array_equal(rec['root_value'][0], o['root_value'], err_msg=f'move {m}: root value')
        np.testing.assert_array_equal(rec['action'][0], o['action'], err_msg=f'move {m}: action')
        for i, e in enumerate(envs):
            _, _, d, _ = e.step(int(rec['action'][0, i]))
            if d:
                e.reset()
    p.close()


def test_learner_gradient_from_the_rings():
    """One HipLearner gradient on a batch of 4 drawn from the ring the device epilogue filled on F: against float64 autograd on the pass's
    own branches at the conv learner's bar, and byte-identical from the int8 ring."""
    from test_gpu_conv_learner import SAME_BRANCH_TOL, _same_branch
    from muzero_amd.hip_learner import HipLearner
    from muzero_amd.replay import Transition

    r = lock_step('F')
    dev = torch.device('cuda', 0)
    n = min(r.counts[-1][('dev', 'f32')], CAP)
    assert n >= 4
    pick = [0, n // 3, n // 2, n - 1]
    out = {}
    for state in ('f32', 'int8'):
        ring_np = r.snap[('dev', state)][0]
        ring = {k: torch.from_numpy(v).to(dev) for k, v in ring_np.items()}
        ring['state'] = ring['state'].reshape(CAP, -1)
        net = _net('F').to(dev)
        net.train()
        hl = HipLearner(net, dev, 5, 4, lr=1e-3)
        idx = torch.tensor(pick, dtype=torch.int64, device=dev)
        loss, prio = hl.grad(ring, idx, None, 4)
        torch.cuda.synchronize()
        out[state] = (hl.grad_flat.cpu().numpy().copy(), loss.cpu().numpy().copy(), prio.cpu().numpy().copy())
        if state == 'f32':
            tr = Transition(*[ring_np[f][pick].reshape((4, 9, 6, 7) if f == 'state' else ring_np[f][pick].shape) for f in Transition._fields])
            w = np.ones(4, np.float32)
            errs, err32, loss_d, _, flipped = _same_branch(hl, net, tr, w, 4, 5, dev)
            assert abs(float(loss) - loss_d) <= 2e-6 * max(1.0, abs(loss_d))
            worst = max(errs, key=errs.get)
            print('worst gradient tensor', worst, errs[worst], 'torch float32 on the same branch', max(err32.values()))
            assert errs[worst] <= SAME_BRANCH_TOL, (worst, errs[worst], flipped)
        hl.close()
    g = out['f32'][0]
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    for x, y, what in zip(out['f32'], out['int8'], ('gradient', 'loss', 'priorities')):
        assert x.tobytes() == y.tobytes(), what


def test_refusals():
    from helpers import build_conv, build_mlp, conv_case, mlp_case
    from muzero_amd import planner as pl
    from muzero_amd.network import MuZeroBoardGameNet

    def refused(p, match, **kw):
        with pytest.raises(pl.PlannerError, match=match):
            p.selfplay_reset_connect4(**kw)
        with pytest.raises(pl.PlannerError, match=match):
            p.arena_reset_connect4('random', **{k: v for k, v in kw.items() if k == 'num_to_win'})

    # an MLP net and an Atari net
    p = pl.Planner(pl.make_mz_config(build_mlp(mlp_case('tictactoe')).planner_spec(), None, num_envs=4, **BOARD_KW), 0)
    refused(p, r'error -1: .*net_kind')
    p.close()
    net = build_conv(conv_case('atari_s'))
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=4), 0)
    refused(p, r'error -1: .*net_kind')
    p.close()
    # num_actions != cols + 1 (a Gomoku net), more than 64 points
    net = build_conv(conv_case('board9'))
    p = _planner(net, 4)
    refused(p, r'error -1: .*num_actions')
    p.close()
    big = MuZeroBoardGameNet((9, 9, 8), 9, 1, 8)
    p = _planner(big, 4)
    refused(p, r'error -1: .*obs_h \* obs_w = 72')
    p.close()
    five = MuZeroBoardGameNet((5, 4, 5), 6, 1, 8)
    p = _planner(five, 4)
    refused(p, r'error -1: .*obs_c')
    p.close()
    # num_to_win out of range; the generic resets; an illegal debug action; external act / commit after this reset
    p = _planner(_net('S'), 4)
    for n in (1, 6, 0, -3):
        refused(p, r'error -1: .*num_to_win', num_to_win=n)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_selfplay_reset_connect4'):
        p.selfplay_reset(pl.ENV_CONNECT4)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_arena_reset_connect4'):
        p.arena_reset(pl.ENV_CONNECT4, 'random')
    with pytest.raises(pl.PlannerError, match=r'error -3: .*mz_selfplay_reset_connect4'):
        p.debug_connect4_step([0, 0, 0, 0])  # before the reset
    p.selfplay_reset_connect4(5)  # 5 = max(rows, cols): the widest legal line
    p.selfplay_reset_connect4(3)
    for _ in range(4):
        p.debug_connect4_step([2, 0, 1, 3])
    before = p.selfplay_counters()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[0\] = 2 is not a legal action of env 0'):
        p.debug_connect4_step([2, 0, 1, 3])  # column 2 of env 0 is full
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[3\] = 6'):
        p.debug_connect4_step([0, 1, 2, 6])
    assert p.selfplay_counters() == before  # refused before any launch
    p._ext_frame = ((9, 4, 5), np.float32)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.external_act(np.zeros((4, 9, 4, 5), np.float32), np.ones((4, 6), np.uint8), 1, 2, 1.0)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.external_commit(np.zeros(4, np.float32), np.zeros(4, np.uint8))
    p.arena_reset_connect4('random', 2, 3)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.debug_connect4_step([0, 0, 0, 0])  # during an arena
    p.close()
    # a frames_u8 replay is not this env's
    from muzero_amd.replay import PrioritizedReplay

    p = _planner(_net('S'), 4)
    rp = PrioritizedReplay(64, 0.0, 0.0, np.random.RandomState(0), device='cuda', state_format='frames_u8', frame_spec=(1, 8, 4, 5, 6))
    p.attach_replay(rp, CFG, obs_shape=(9, 4, 5))
    with pytest.raises(pl.PlannerError, match=r'error -1: .*state_format'):
        p.selfplay_reset_connect4(3)
    p.close()


def test_run_self_play_by_name_is_the_host_loop():
    """pipeline.run_self_play(env='ConnectFour') on the device emits the items the same call emits over a list of host ConnectFourEnv
    objects (the host-stepped path), into a queue and into a device replay."""
    import queue

    from muzero_amd import pipeline
    from muzero_amd.config import make_connect4_config
    from muzero_amd.games import ConnectFourEnv
    from muzero_amd.replay import PrioritizedReplay

    B, M = 8, 32
    net = _net('F')
    never = types.SimpleNamespace(is_set=lambda: False)
    out = {}
    for where in ('device', 'host'):
        for sink in ('queue', 'replay'):
            cfg = make_connect4_config(num_simulations=SIMS)
            cfg.num_envs = B
            env = 'ConnectFour' if where == 'device' else [ConnectFourEnv() for _ in range(B)]
            q = queue.Queue() if sink == 'queue' else PrioritizedReplay(512, 0.0, 0.0, np.random.RandomState(0), device='cuda')
            steps = pipeline.run_self_play(cfg, 0, net, torch.device('cuda', 0), env, q, types.SimpleNamespace(value=0), never, max_moves=M)
            assert steps == B * M
            if sink == 'queue':
                items = []
                while not q.empty():
                    items.append(q.get())
                out[(where, sink)] = items
            else:
                st = q.get_state()
                n = min(st['num_added'], q.capacity)
                out[(where, sink)] = (st['num_added'], {f: st['storage'][f][:n].numpy() for f in ('state', 'action', 'pi_prob', 'value', 'reward')})
    a, b = out[('device', 'queue')], out[('host', 'queue')]
    assert len(a) == len(b) > B
    for (t0, p0), (t1, p1) in zip(a, b):
        assert p0 == p1
        for f in ('state', 'action', 'pi_prob', 'value', 'reward'):
            x, y = getattr(t0, f), getattr(t1, f)
            assert x.dtype == y.dtype and np.array_equal(x, y), f
    (n0, f0), (n1, f1) = out[('device', 'replay')], out[('host', 'replay')]
    assert n0 == n1 == len(a)
    for f in f0:
        assert np.array_equal(f0[f], f1[f]), f
