"""The device Othello env (mz_selfplay_reset_othello, csrc/mz_othello.h) on an MI355X, held to `games.OthelloEnv` byte for byte: the
scripted games of othello_cases.py through the debug step, several side by side with auto-resets; searched self-play in lock-step with a
host-stepped planner fed by host envs, records and replay rings (float32 and int8) identical; n moves in one call; the searches against
the oracle; one HipLearner gradient from the rings at 18 and 26 actions; run_self_play by name; the refusals."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import othello_cases as oc
from helpers import seeded_state_dict

pytestmark = pytest.mark.gpu

REC = ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')
BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
CFG = types.SimpleNamespace(is_board_game=True, acc_seq_length=9999, unroll_steps=5, td_steps=0, discount=1.0)
# The lock-step runs: shape -> (envs, moves, planner seed).  A seed is kept if its run meets the conditions test_lock_step_self_play
# asserts from the host envs' own records (a searched pass, an auto-reset in the middle of the others' games).
LOCK = {'S': (8, 40, 8), 'N': (8, 40, 12), 'F': (8, 24, 1)}  # (of seeds 1 .. 12: S 3, 8 .. 12 and N 2, 4, 9, 12 hold a pass)
SIMS = 8


def _net(shape, planes=8, blocks=1, seed=31):
    from muzero_amd.network import MuZeroBoardGameNet

    rows, cols = oc.SHAPES[shape]
    net = MuZeroBoardGameNet((9, rows, cols), rows * cols + 2, blocks, planes)
    net.load_state_dict(seeded_state_dict(net, seed + rows + cols))
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


@pytest.mark.parametrize('shape', ['S', 'N', 'M', 'F'])
def test_scripted_games_on_the_kernel(shape):
    """Every scripted game of the shape as one env of one planner, played through the debug step beside a host env.  An env plays its
    game again and again (a game that does not end by itself is ended by a resignation), so the envs finish at different plies and reset
    while their neighbours play on.  After every ply the record, the mask, the counters and the next observation equal the host's."""
    rows, cols = oc.SHAPES[shape]
    nn, A = rows * cols, rows * cols + 2
    games = oc.cases(shape)
    scripts = [c['moves'] + ([] if c['done'] else [nn + 1]) for c in games]
    B, plies = len(games), max(len(s) for s in scripts) + 12
    p = _planner(_net(shape), B)
    rp = _replay(4096, 'f32')
    p.attach_replay(rp, CFG, obs_shape=(9, rows, cols))
    p.selfplay_reset_othello()
    envs = [oc.make_env(shape) for _ in range(B)]
    at = [0] * B
    movers, returns = [[] for _ in range(B)], []  # the Monte-Carlo returns the epilogue must write, in its order (move, then env)
    episodes = steps_done = 0
    ends = []
    assert np.array_equal(p.debug_othello_mask(), np.stack([e.actions_mask for e in envs]).astype(np.uint8))
    for ply in range(plies):
        obs = np.stack([e.observation() for e in envs]).astype(np.float32).reshape(B, -1)
        players = np.array([e.current_player for e in envs], np.int32)
        acts = np.array([scripts[i][at[i]] for i in range(B)], np.int32)
        p.debug_othello_step(acts)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for i, e in enumerate(envs):
            movers[i].append(e.current_player)
            _, rew[i], d, _ = e.step(int(acts[i]))
            if d:  # +1 / 0 / -1 by the count or -1 by resignation, seen from each ply's mover
                returns += [float(rew[i]) * (1.0 if m == movers[i][-1] else -1.0) for m in movers[i]]
                movers[i] = []
            if at[i] < len(games[i]['boards']):
                assert np.array_equal(e.board, oc.board_array(games[i]['boards'][at[i]]))
            at[i] += 1
            if d:
                assert at[i] == len(scripts[i]), (games[i]['name'], ply)  # the game ended where its case says, not before
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
        assert np.array_equal(rec['pi'][0], np.eye(A)[acts]) and not rec['root_value'][0].any()
        assert np.array_equal(p.debug_othello_mask(), np.stack([e.actions_mask for e in envs]).astype(np.uint8)), ply
        assert np.array_equal(p.debug_othello_board(), np.stack([e.board.reshape(-1) for e in envs])), ply
        c = p.selfplay_counters()
        assert (c['env_steps'], c['simulations'], c['episodes'], c['episode_steps']) == (B * (ply + 1), 0, episodes, steps_done), (ply, c)
    ends = np.stack(ends)
    assert ends.any(axis=0).all()  # every game was played to its end
    p.synchronize()
    assert rp.num_added == len(returns) == steps_done <= 4096
    np.testing.assert_array_equal(rp._ring['value'].cpu().numpy()[:len(returns), 0], np.array(returns, np.float32))
    assert {-1.0, 0.0, 1.0} <= set(returns) or shape in 'MF'  # ends by the count both ways and a draw, through the epilogue
    assert episodes >= 2 * B and len({int(np.flatnonzero(ends[:, i])[0]) for i in range(B)}) >= min(4, B)  # the envs finish at different plies
    # the state after the last ply (fresh boards where a game has just ended) is what the next record shows
    obs = np.stack([e.observation() for e in envs]).astype(np.float32).reshape(B, -1)
    p.debug_othello_step(np.array([int(np.flatnonzero(e.actions_mask)[0]) for e in envs], np.int32))
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
    """A device Othello planner and a host-stepped planner fed by host OthelloEnv objects, for each replay state format (none, float32,
    int8), same seed, stepped in lock-step with the board temperature schedule.  Everything the tests below read."""
    B, M, picked = LOCK[shape]
    seed = picked if seed is None else seed
    rows, cols = oc.SHAPES[shape]
    nn = rows * cols
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
                p.selfplay_reset_othello()
            else:
                p.selfplay_reset_external(frame_shape=(9, rows, cols), temp_switch_steps=6, max_episode_steps=2 * (nn - 4))
            side[(where, state)] = (p, rp, origin)
    envs = [oc.make_env(shape) for _ in range(B)]
    obs = [e.reset() for e in envs]
    base = ('host', None)
    equal, actions_equal, dones, counts = [], [], [], []
    lengths, passes, mid_game, final_rewards = [], 0, False, []
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
            a = int(acts[base][i])
            passes += a == nn
            obs[i], rew[i], d, _ = e.step(a)
            if d:
                lengths.append(e.steps)
                final_rewards.append((a, float(rew[i])))
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
                                 counters=counters, snap=snap, base=base, lengths=lengths, passes=passes, mid_game=mid_game,
                                 final_rewards=final_rewards, net=net, shape=shape)


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    lock_step.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('shape', ['S', 'N', 'F'])
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
    print('episode lengths', r.lengths, 'searched passes', r.passes, 'final (action, reward)', r.final_rewards)
    if shape != 'F':  # the run shows something: a searched pass, and episodes that ended and reset while others played on
        assert r.passes >= 1, r.passes
        assert len(r.lengths) >= 1 and r.mid_game, r.lengths


@pytest.mark.parametrize('shape', ['S', 'N'])
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


@pytest.mark.parametrize('shape', ['S', 'N', 'F'])
def test_n_moves_in_one_call(shape):
    """n moves in one mz_selfplay_step equal n calls of one, and both are the lock-step run's device side."""
    B, M, seed = LOCK[shape]
    r = lock_step(shape)
    out = []
    for chunks in ([1] * M, [7, 1, M - 8]):
        p = _planner(r.net, B, seed=seed)
        rp = _replay(CAP, 'int8')
        origin = p.attach_replay(rp, CFG, obs_shape=(9,) + oc.SHAPES[shape], with_origin=True)
        p.selfplay_reset_othello()
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


@pytest.mark.parametrize('shape', ['S', 'N'])
def test_self_play_search_equals_the_oracle(oracle, shape):
    """3 moves of 4 envs: the recorded observation, the host env's mask and players and the captured Philox draws through
    oracle.uct_search_batch give the device move's policy (the visit distribution: temperature 1 in the first moves), root value and
    action -- on a mask the env rebuilt from the whole position, with rows * cols + 2 actions."""
    from test_oracle_nets import _oracle_net

    rows, cols = oc.SHAPES[shape]
    B, A = 4, rows * cols + 2
    net = _net(shape)
    p = _planner(net, B, seed=77, capture=True)
    p.selfplay_reset_othello()
    onet = _oracle_net(oracle, net, 'conv')
    cfg = oracle.make_config(A, SIMS, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    envs = [oc.make_env(shape) for _ in range(B)]
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
        # (the first simulation ties every action, illegal ones included: visits that fell on illegal actions are not in the policy)
        np.testing.assert_array_equal(np.rint(rec['pi'][0] * o['visits'].sum(axis=1, keepdims=True)), o['visits'], err_msg=f'move {m}: visit counts')
        np.testing.assert_array_equal(rec['pi'][0], o['pi'], err_msg=f'move {m}: policy')
        np.testing.assert_array_equal(rec['root_value'][0], o['root_value'], err_msg=f'move {m}: root value')
        np.testing.assert_array_equal(rec['action'][0], o['action'], err_msg=f'move {m}: action')
        for i, e in enumerate(envs):
            _, _, d, _ = e.step(int(rec['action'][0, i]))
            if d:
                e.reset()
    p.close()


@pytest.mark.parametrize('shape', ['S', 'N'])
def test_learner_gradient_from_the_rings(shape):
    """One HipLearner gradient on a batch of 4 drawn from the ring the device epilogue filled, at (9, 4, 4) / 18 actions and (9, 4, 6) /
    26 -- the first board nets whose action count exceeds their point count + 1: against float64 autograd on the pass's own branches at
    the conv learner's bar (the one tests/test_gpu_connect4.py uses), and byte-identical from the int8 ring."""
    from test_gpu_conv_learner import SAME_BRANCH_TOL, _same_branch
    from muzero_amd.hip_learner import HipLearner
    from muzero_amd.replay import Transition

    rows, cols = oc.SHAPES[shape]
    r = lock_step(shape)
    dev = torch.device('cuda', 0)
    n = min(r.counts[-1][('dev', 'f32')], CAP)
    assert n >= 4
    pick = [0, n // 3, n // 2, n - 1]
    out = {}
    for state in ('f32', 'int8'):
        ring_np = r.snap[('dev', state)][0]
        ring = {k: torch.from_numpy(v).to(dev) for k, v in ring_np.items()}
        ring['state'] = ring['state'].reshape(CAP, -1)
        net = _net(shape).to(dev)
        net.train()
        hl = HipLearner(net, dev, 5, 4, lr=1e-3)
        idx = torch.tensor(pick, dtype=torch.int64, device=dev)
        loss, prio = hl.grad(ring, idx, None, 4)
        torch.cuda.synchronize()
        out[state] = (hl.grad_flat.cpu().numpy().copy(), loss.cpu().numpy().copy(), prio.cpu().numpy().copy())
        if state == 'f32':
            tr = Transition(*[ring_np[f][pick].reshape((4, 9, rows, cols) if f == 'state' else ring_np[f][pick].shape) for f in Transition._fields])
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

    def refused(p, match):
        with pytest.raises(pl.PlannerError, match=match):
            p.selfplay_reset_othello()
        with pytest.raises(pl.PlannerError, match=match):
            p.arena_reset_othello('random')

    # an MLP net and an Atari net
    p = pl.Planner(pl.make_mz_config(build_mlp(mlp_case('tictactoe')).planner_spec(), None, num_envs=4, **BOARD_KW), 0)
    refused(p, r'error -1: .*net_kind')
    p.close()
    net = build_conv(conv_case('atari_s'))
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=4), 0)
    refused(p, r'error -1: .*net_kind')
    p.close()
    # num_actions != rows * cols + 2 (a Gomoku net), boards outside 4 .. 8, the wrong plane count
    net = build_conv(conv_case('board9'))
    p = _planner(net, 4)
    refused(p, r'error -1: .*(num_actions|obs_h|obs_w)')
    p.close()
    for shape, field in (((9, 3, 6), 'obs_h'), ((9, 9, 6), 'obs_h'), ((9, 6, 3), 'obs_w'), ((9, 6, 9), 'obs_w')):
        p = _planner(MuZeroBoardGameNet(shape, shape[1] * shape[2] + 2, 1, 8), 4)
        refused(p, r'error -1: .*' + field)
        p.close()
    p = _planner(MuZeroBoardGameNet((9, 4, 4), 17, 1, 8), 4)
    refused(p, r'error -1: .*num_actions must be obs_h \* obs_w \+ 2 = 18')
    p.close()
    p = _planner(MuZeroBoardGameNet((5, 4, 4), 18, 1, 8), 4)
    refused(p, r'error -1: .*obs_c')
    p.close()
    # the generic resets; an illegal debug action; external act / commit after this reset
    p = _planner(_net('S'), 4)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_selfplay_reset_othello'):
        p.selfplay_reset(pl.ENV_OTHELLO)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_arena_reset_othello'):
        p.arena_reset(pl.ENV_OTHELLO, 'random')
    with pytest.raises(pl.PlannerError, match=r'error -3: .*mz_selfplay_reset_othello'):
        p.debug_othello_step([1, 1, 1, 1])  # before the reset
    with pytest.raises(pl.PlannerError, match=r'error -3: .*mz_othello_debug_board'):
        p.debug_othello_board()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*temp_switch_steps'):
        p.selfplay_reset_othello(-1)
    p.selfplay_reset_othello()
    p.debug_othello_step([1, 4, 11, 14])
    before = p.selfplay_counters()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[0\] = 1 is not a legal action of env 0'):
        p.debug_othello_step([1, 0, 0, 0])  # occupied
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[2\] = 16'):
        p.debug_othello_step([0, 0, 16, 17])  # env 2 has placements: no pass
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[3\] = 18'):
        p.debug_othello_step([17, 17, 17, 18])
    assert p.selfplay_counters() == before  # refused before any launch
    p._ext_frame = ((9, 4, 4), np.float32)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.external_act(np.zeros((4, 9, 4, 4), np.float32), np.ones((4, 18), np.uint8), 1, 2, 1.0)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.external_commit(np.zeros(4, np.float32), np.zeros(4, np.uint8))
    p.arena_reset_othello('random', 2)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.debug_othello_step([0, 0, 0, 0])  # during an arena
    p.close()
    # a frames_u8 replay is not this env's
    from muzero_amd.replay import PrioritizedReplay

    p = _planner(_net('S'), 4)
    rp = PrioritizedReplay(64, 0.0, 0.0, np.random.RandomState(0), device='cuda', state_format='frames_u8', frame_spec=(1, 8, 4, 4, 18))
    p.attach_replay(rp, CFG, obs_shape=(9, 4, 4))
    with pytest.raises(pl.PlannerError, match=r'error -1: .*state_format'):
        p.selfplay_reset_othello()
    p.close()


def test_run_self_play_by_name_is_the_host_loop():
    """pipeline.run_self_play(env='Othello') on the device emits the items the same call emits over a list of host OthelloEnv objects
    (the host-stepped path), into a queue and into a device replay."""
    import queue

    from muzero_amd import pipeline
    from muzero_amd.config import make_othello_config
    from muzero_amd.games import OthelloEnv
    from muzero_amd.replay import PrioritizedReplay

    B, M = 8, 32
    net = _net('N')
    never = types.SimpleNamespace(is_set=lambda: False)
    out = {}
    for where in ('device', 'host'):
        for sink in ('queue', 'replay'):
            cfg = make_othello_config(rows=4, cols=6, num_simulations=SIMS)
            cfg.num_envs = B
            env = 'Othello' if where == 'device' else [OthelloEnv(4, 6) for _ in range(B)]
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
