"""The device Go env (mz_selfplay_reset_go, csrc/mz_go.h) on an MI355X, held to `games.GoEnv` byte for byte: the scripted games of
go_cases.py through the debug step, several side by side with auto-resets, boards and masks after every ply; searched self-play in
lock-step with a host-stepped planner fed by host envs, records and replay rings (float32 and int8) identical; n moves in one call; the
searches against the oracle; one HipLearner gradient from the rings at 27 and 83 actions; run_self_play by name; the refusals."""
import ctypes as C
import functools
import types

import numpy as np
import pytest
import torch

import go_cases as gc
from helpers import seeded_state_dict
from muzero_amd.games import GoEnv

pytestmark = pytest.mark.gpu

REC = ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')
BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
CFG = types.SimpleNamespace(is_board_game=True, acc_seq_length=9999, unroll_steps=5, td_steps=0, discount=1.0)
SIMS = 8
# The lock-step runs: name -> (rows, cols, rules, envs, moves, planner seed).  max_plies is small so that games end, by the count, inside
# the run and their items reach the replay; where the resignation is allowed the searches take it too.
LOCK = {
    '5x5': (5, 5, dict(komi2=15, max_plies=14, allow_resign=True), 8, 40, 8),
    '5x5-no-resign': (5, 5, dict(komi2=3, max_plies=12, allow_resign=False), 8, 30, 3),
    '4x6': (4, 6, dict(komi2=15, max_plies=14, allow_resign=True), 8, 40, 12),
    '4x6-no-resign': (4, 6, dict(komi2=4, max_plies=12, allow_resign=False), 8, 30, 5),
    '9x9': (9, 9, dict(komi2=15, max_plies=10, allow_resign=True), 4, 24, 2),
    '19x19': (19, 19, dict(komi2=15, max_plies=0, allow_resign=True), 2, 6, 1),
}


def _net(rows, cols, planes=8, blocks=1, seed=31):
    from muzero_amd.network import MuZeroBoardGameNet

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


def _replay(cap, state):
    from muzero_amd.replay import PrioritizedReplay

    kw = dict(state_format='int8') if state == 'int8' else {}
    return PrioritizedReplay(cap, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw)


GROUPS = gc.groups()


@pytest.mark.parametrize('key', list(GROUPS), ids=[f'{k[0]}x{k[1]}-' + '-'.join(str(v) for _, v in k[2:]) for k in GROUPS])
def test_scripted_games_on_the_kernel(key):
    """Every scripted game of one board and rule set as one env of one planner, played through the debug step beside a host env.  An env
    plays its game again and again (a game that does not end by itself is ended by a resignation), so the envs finish at different plies
    and reset while their neighbours play on.  After every ply the device board equals the hand-written one, and the record, the mask,
    the counters and the next observation equal the host's; at the end the replay holds the Monte-Carlo returns."""
    games = GROUPS[key]
    rows, cols, rules = key[0], key[1], dict(key[2:])
    nn, A = rows * cols, rows * cols + 2
    scripts = [[gc.action_of(c, ply[0]) for ply in c['plies']] + ([] if c['end'] is not None else [nn + 1]) for c in games]
    B, longest = len(games), max(len(s) for s in scripts)
    plies = longest + (12 if longest < 100 else 1)
    p = _planner(_net(rows, cols), B)
    rp = _replay(4096, 'f32')
    p.attach_replay(rp, CFG, obs_shape=(9, rows, cols))
    p.selfplay_reset_go(**rules)
    envs = [GoEnv(rows, cols, **rules) for _ in range(B)]
    at = [0] * B
    movers, returns = [[] for _ in range(B)], []  # the Monte-Carlo returns the epilogue must write, in its order (move, then env)
    episodes = steps_done = 0
    ends = []
    assert np.array_equal(p.debug_go_mask(), np.stack([e.actions_mask for e in envs]).astype(np.uint8))
    for ply in range(plies):
        obs = np.stack([e.observation() for e in envs]).astype(np.float32).reshape(B, -1)
        players = np.array([e.current_player for e in envs], np.int32)
        acts = np.array([scripts[i][at[i]] for i in range(B)], np.int32)
        p.debug_go_step(acts)
        board = p.debug_go_board()
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for i, e in enumerate(envs):
            movers[i].append(e.current_player)
            _, rew[i], d, _ = e.step(int(acts[i]))
            if d:  # +1 / 0 / -1 by the count or -1 by resignation, seen from each ply's mover
                returns += [float(rew[i]) * (1.0 if m == movers[i][-1] else -1.0) for m in movers[i]]
                movers[i] = []
            if at[i] < len(games[i]['plies']) and not d:  # the hand-written board, straight against the device's
                assert np.array_equal(board[i], gc.parse(games[i]['plies'][at[i]][1]).reshape(-1)), (games[i]['name'], at[i] + 1)
            at[i] += 1
            if d:
                assert at[i] == len(scripts[i]), (games[i]['name'], ply)  # the game ended where its case says, not before
                if games[i]['end'] is not None:
                    assert (float(rew[i]), e.winner) == games[i]['end'], games[i]['name']
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
        assert np.array_equal(p.debug_go_mask(), np.stack([e.actions_mask for e in envs]).astype(np.uint8)), ply
        assert np.array_equal(board, np.stack([e.board.reshape(-1) for e in envs])), ply
        c = p.selfplay_counters()
        assert (c['env_steps'], c['simulations'], c['episodes'], c['episode_steps']) == (B * (ply + 1), 0, episodes, steps_done), (ply, c)
    ends = np.stack(ends)
    assert ends.any(axis=0).all()  # every game was played to its end
    p.synchronize()
    assert rp.num_added == len(returns) == steps_done <= 4096
    np.testing.assert_array_equal(rp._ring['value'].cpu().numpy()[:len(returns), 0], np.array(returns, np.float32))
    # the state after the last ply (fresh boards where a game has just ended) is what the next record shows
    obs = np.stack([e.observation() for e in envs]).astype(np.float32).reshape(B, -1)
    p.debug_go_step(np.full(B, nn, np.int32))
    assert p.selfplay_read(1)['obs'][0].tobytes() == obs.tobytes()
    p.close()


def _snap(rp, origin):
    torch.cuda.synchronize()
    return ({k: v.cpu().numpy().copy() for k, v in rp._ring.items()}, rp._attached[0].cpu().numpy().copy(), origin.cpu().numpy().copy())


CAP = 96


@functools.lru_cache(maxsize=None)
def lock_step(name):
    """A device Go planner and a host-stepped planner fed by host GoEnv objects, for each replay state format (none, float32, int8), same
    seed, stepped in lock-step with the board temperature schedule.  Everything the tests below read."""
    rows, cols, rules, B, M, seed = LOCK[name]
    nn = rows * cols
    net = _net(rows, cols)
    side = {}
    for where in ('host', 'dev'):
        for state in (None, 'f32', 'int8'):
            p = _planner(net, B, seed=seed)
            rp = origin = None
            if state is not None:
                rp = _replay(CAP, state)
                origin = p.attach_replay(rp, CFG, obs_shape=(9, rows, cols), with_origin=True)
            if where == 'dev':
                p.selfplay_reset_go(**rules)
            else:
                p.selfplay_reset_external(frame_shape=(9, rows, cols), temp_switch_steps=6, max_episode_steps=rules['max_plies'] or 2 * nn)
            side[(where, state)] = (p, rp, origin)
    envs = [GoEnv(rows, cols, **rules) for _ in range(B)]
    obs = [e.reset() for e in envs]
    base = ('host', None)
    equal, actions_equal, dones, counts = [], [], [], []
    lengths, passes, resigns, captures, final_rewards = [], 0, 0, 0, []
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
            resigns += a == nn + 1
            stones = np.count_nonzero(e.board)
            obs[i], rew[i], d, _ = e.step(a)
            captures += a < nn and np.count_nonzero(e.board) <= stones
            if d:
                lengths.append(e.steps)
                final_rewards.append((a, float(rew[i])))
                obs[i] = e.reset()
            done[i] = d
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
                                 counters=counters, snap=snap, base=base, lengths=lengths, passes=passes, resigns=resigns, captures=captures,
                                 final_rewards=final_rewards, net=net, rules=rules, rows=rows, cols=cols)


@pytest.fixture(scope='module', autouse=True)
def _release():
    yield
    lock_step.cache_clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize('name', list(LOCK))
def test_lock_step_self_play(name):
    r = lock_step(name)
    assert all(r.actions_equal), [m for m, ok in enumerate(r.actions_equal) if not ok]
    for k in r.side:
        assert all(eq[k] for eq in r.equal), (k, [m for m, eq in enumerate(r.equal) if not eq[k]])
        for f in REC:
            assert r.last[k][f].tobytes() == r.last[r.base][f].tobytes(), (k, f)
        assert r.counters[k] == r.counters[r.base], k
    c = r.counters[r.base]
    assert c['env_steps'] == r.M * r.B and c['simulations'] == r.M * r.B * SIMS and c['episodes'] == r.dones.sum() == len(r.lengths)
    assert c['episode_steps'] == sum(r.lengths)
    print('episode lengths', r.lengths, 'searched passes', r.passes, 'resignations', r.resigns, 'capturing plies', r.captures,
          'final (action, reward)', r.final_rewards)
    if not r.rules['allow_resign']:
        assert r.resigns == 0
    if r.rules['max_plies']:  # every env ends a game by max_plies at the latest
        assert len(r.lengths) >= r.B * (r.M // r.rules['max_plies']) and max(r.lengths) <= r.rules['max_plies']


@pytest.mark.parametrize('name', ['5x5', '5x5-no-resign', '4x6', '4x6-no-resign', '9x9'])
def test_replay_rings_are_byte_identical(name):
    r = lock_step(name)
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


@pytest.mark.parametrize('name', ['5x5', '4x6-no-resign', '19x19'])
def test_n_moves_in_one_call(name):
    """n moves in one mz_selfplay_step equal n calls of one, and both are the lock-step run's device side."""
    rows, cols, rules, B, M, seed = LOCK[name]
    r = lock_step(name)
    out = []
    for chunks in ([1] * M, [3, 1, M - 4]):
        p = _planner(r.net, B, seed=seed)
        rp = _replay(CAP, 'int8')
        origin = p.attach_replay(rp, CFG, obs_shape=(9, rows, cols), with_origin=True)
        p.selfplay_reset_go(**rules)
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


@pytest.mark.parametrize('rows,cols', [(5, 5), (4, 6)])
def test_self_play_search_equals_the_oracle(oracle, rows, cols):
    """3 moves of 4 envs: the recorded observation, the host env's mask and players and the captured Philox draws through
    oracle.uct_search_batch give the device move's policy, root value and action -- on a mask the env rebuilt from the whole position,
    with rows * cols + 2 actions.  (7 x 11, a non-square board above 64 points, is refused at the reset: test_refusals.)"""
    from test_oracle_nets import _oracle_net

    B, A = 4, rows * cols + 2
    net = _net(rows, cols)
    p = _planner(net, B, seed=77, capture=True)
    p.selfplay_reset_go()
    onet = _oracle_net(oracle, net, 'conv')
    cfg = oracle.make_config(A, SIMS, 1.0, True, (-1.0, 1.0), 0.25, 0.25)
    envs = [GoEnv(rows, cols) for _ in range(B)]
    checked = 0
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
        # The first simulation ties every action, illegal ones included; with 8 simulations and a peaked net every visit can then fall
        # on one occupied point, and the oracle's policy is the reference's 0 / 0 (known deviation: device self-play plays
        # uniformly over the legal moves there instead of stopping the actor).  Such a row is held to exactly that; on the empty board
        # (move 0) there is none, and no run may consist of them.
        lost = np.isnan(o['pi']).any(axis=1)
        ok = ~lost
        assert not (lost.any() and m == 0) and ok.sum() >= B - 1, (m, lost)  # at most one such row in a move
        for i in np.flatnonzero(lost):
            assert o['visits'][i].sum() == 0 and mask[i, rec['action'][0, i]]
            np.testing.assert_array_equal(rec['pi'][0, i], mask[i] / mask[i].sum(), err_msg=f'move {m}, env {i}: uniform over the legal moves')
        checked += int(ok.sum())
        np.testing.assert_array_equal(np.rint(rec['pi'][0] * o['visits'].sum(axis=1, keepdims=True))[ok], o['visits'][ok], err_msg=f'move {m}: visit counts')
        np.testing.assert_array_equal(rec['pi'][0][ok], o['pi'][ok], err_msg=f'move {m}: policy')
        np.testing.assert_array_equal(rec['root_value'][0][ok], o['root_value'][ok], err_msg=f'move {m}: root value')
        np.testing.assert_array_equal(rec['action'][0][ok], o['action'][ok], err_msg=f'move {m}: action')
        for i, e in enumerate(envs):
            _, _, d, _ = e.step(int(rec['action'][0, i]))
            if d:
                e.reset()
    p.close()
    print('rows held to the oracle', checked, 'of', 3 * B)
    assert checked >= 3 * B - 1  # and at most one in the run: eleven of twelve searches at the least equal the oracle's


@pytest.mark.parametrize('name', ['5x5', '9x9'])
def test_learner_gradient_from_the_rings(name):
    """One HipLearner gradient on a batch of 4 drawn from the ring the device epilogue filled, at (9, 5, 5) / 27 actions and (9, 9, 9) /
    83: against float64 autograd on the pass's own branches at the conv learner's bar (the one tests/test_gpu_connect4.py uses), and
    byte-identical from the int8 ring."""
    from test_gpu_conv_learner import SAME_BRANCH_TOL, _same_branch
    from muzero_amd.hip_learner import HipLearner
    from muzero_amd.replay import Transition

    r = lock_step(name)
    rows, cols = r.rows, r.cols
    dev = torch.device('cuda', 0)
    n = min(r.counts[-1][('dev', 'f32')], CAP)
    assert n >= 4
    pick = [0, n // 3, n // 2, n - 1]
    out = {}
    for state in ('f32', 'int8'):
        ring_np = r.snap[('dev', state)][0]
        ring = {k: torch.from_numpy(v).to(dev) for k, v in ring_np.items()}
        ring['state'] = ring['state'].reshape(CAP, -1)
        net = _net(rows, cols).to(dev)
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

    def refused(p, match, **kw):
        with pytest.raises(pl.PlannerError, match=match):
            p.selfplay_reset_go(**kw)
        with pytest.raises(pl.PlannerError, match=match):
            p.arena_reset_go('random', **kw)

    # an MLP net and an Atari net
    p = pl.Planner(pl.make_mz_config(build_mlp(mlp_case('tictactoe')).planner_spec(), None, num_envs=4, **BOARD_KW), 0)
    refused(p, r'error -1: .*net_kind')
    p.close()
    net = build_conv(conv_case('atari_s'))
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=4), 0)
    refused(p, r'error -1: .*net_kind')
    p.close()
    # num_actions != rows * cols + 2 (a Gomoku net), boards outside 3 .. 19, a non-square board above 64 points, the wrong plane count
    p = _planner(build_conv(conv_case('board9')), 4)
    refused(p, r'error -1: .*num_actions')
    p.close()
    for shape, field in (((9, 2, 6), 'obs_h'), ((9, 20, 6), 'obs_h'), ((9, 6, 2), 'obs_w'), ((9, 6, 20), 'obs_w')):
        p = _planner(MuZeroBoardGameNet(shape, shape[1] * shape[2] + 2, 1, 8), 4)
        refused(p, r'error -1: .*' + field)
        p.close()
    p = _planner(MuZeroBoardGameNet((9, 7, 11), 79, 1, 8), 4)
    refused(p, r'error -1: .*7 x 11.*more than 64 points must be square')
    p.close()
    p = _planner(MuZeroBoardGameNet((9, 5, 5), 26, 1, 8), 4)
    refused(p, r'error -1: .*num_actions must be obs_h \* obs_w \+ 2 = 27')
    p.close()
    p = _planner(MuZeroBoardGameNet((5, 5, 5), 27, 1, 8), 4)
    refused(p, r'error -1: .*obs_c')
    p.close()
    # the rules; the generic resets; an illegal debug action; external act / commit after this reset
    p = _planner(_net(5, 5), 4)
    refused(p, r'error -1: .*komi2', komi2=-1)
    refused(p, r'error -1: .*komi2', komi2=51)
    refused(p, r'error -1: .*max_plies', max_plies=-1)
    refused(p, r'error -1: .*max_plies', max_plies=51)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_selfplay_reset_go'):
        p.selfplay_reset(pl.ENV_GO)
    with pytest.raises(pl.PlannerError, match=r'error -1: .*mz_arena_reset_go'):
        p.arena_reset(pl.ENV_GO, 'random')
    with pytest.raises(pl.PlannerError, match=r'error -3: .*mz_selfplay_reset_go'):
        p.debug_go_step([1, 1, 1, 1])  # before the reset
    with pytest.raises(pl.PlannerError, match=r'error -3: .*mz_go_debug_board'):
        p.debug_go_board()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*temp_switch_steps'):
        p.selfplay_reset_go(temp_switch_steps=-1)
    p.selfplay_reset_go(allow_resign=False)
    p.debug_go_step([0, 6, 12, 25])
    before = p.selfplay_counters()
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[0\] = 0 is not a legal action of env 0'):
        p.debug_go_step([0, 0, 0, 0])  # occupied
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[2\] = 26'):
        p.debug_go_step([1, 1, 26, 26])  # the resignation is off
    with pytest.raises(pl.PlannerError, match=r'error -1: .*h_action\[3\] = 27'):
        p.debug_go_step([25, 25, 25, 27])
    assert p.selfplay_counters() == before  # refused before any launch
    # an arena reset that is refused for its sides leaves the running game's rules alone: the resignation stays off
    with pytest.raises(pl.PlannerError, match=r'error -1: .*opening_plies'):
        p.arena_reset_go('random', -1, komi2=3, max_plies=7, allow_resign=True)
    p.debug_go_step([1, 1, 1, 1])
    assert not p.debug_go_mask()[:, 26].any() and p.selfplay_counters()['episodes'] == 0
    p._ext_frame = ((9, 5, 5), np.float32)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.external_act(np.zeros((4, 9, 5, 5), np.float32), np.ones((4, 27), np.uint8), 1, 2, 1.0)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.external_commit(np.zeros(4, np.float32), np.zeros(4, np.uint8))
    p.arena_reset_go('random', 2)
    with pytest.raises(pl.PlannerError, match=r'error -3: '):
        p.debug_go_step([0, 0, 0, 0])  # during an arena
    p.close()
    # a frames_u8 replay is not this env's
    from muzero_amd.replay import PrioritizedReplay

    p = _planner(_net(5, 5), 4)
    rp = PrioritizedReplay(64, 0.0, 0.0, np.random.RandomState(0), device='cuda', state_format='frames_u8', frame_spec=(1, 8, 5, 5, 27))
    p.attach_replay(rp, CFG, obs_shape=(9, 5, 5))
    with pytest.raises(pl.PlannerError, match=r'error -1: .*state_format'):
        p.selfplay_reset_go()
    p.close()


def test_run_self_play_by_name_is_the_host_loop():
    """pipeline.run_self_play(env='Go') on the device emits the items the same call emits over a list of host GoEnv objects (the
    host-stepped path), into a queue and into a device replay; the rules come off the config for the name and off the env objects."""
    import queue

    from muzero_amd import pipeline
    from muzero_amd.config import make_go_config
    from muzero_amd.replay import PrioritizedReplay

    B, M = 8, 32
    net = _net(4, 6)
    never = types.SimpleNamespace(is_set=lambda: False)
    out = {}
    for where in ('device', 'host'):
        for sink in ('queue', 'replay'):
            cfg = make_go_config(rows=4, cols=6, num_simulations=SIMS, komi2=5, max_plies=12, allow_resign=False, temp_switch_steps=6)
            cfg.num_envs = B
            env = 'Go' if where == 'device' else [GoEnv(4, 6, komi2=5, max_plies=12, allow_resign=False) for _ in range(B)]
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
