"""Self-play on host-stepped environments (mz_selfplay_reset_external / _act / _commit, pipeline.run_self_play with env objects):
the same games played by host env objects and by the device environments give the same records and replay items bit for bit,
device frame stacking equals host stacking (StackFrameAndAction, ScaledFloatFrame), and every misuse returns its error code."""
import queue
import types

import numpy as np
import pytest
import torch

from helpers import build_conv, build_mlp, conv_case, mlp_case

pytestmark = pytest.mark.gpu

FIELDS = ('state', 'action', 'pi_prob', 'value', 'reward')
REC = ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')


def _never():
    return types.SimpleNamespace(is_set=lambda: False)


def _replay_contents(rp):
    from muzero_amd.replay import PrioritizedReplay

    assert isinstance(rp, PrioritizedReplay)
    st = rp.get_state()
    n = min(st['num_added'], rp.capacity)
    return st['num_added'], {f: st['storage'][f][:n].numpy() for f in FIELDS}, np.asarray(st['priorities'][:n])


def _tictactoe_cfg(B):
    from muzero_amd.config import make_tictactoe_config

    cfg = make_tictactoe_config(use_tensorboard=False)
    cfg.num_envs = B
    return cfg


def test_tictactoe_host_envs_equal_device_env_into_device_replay():
    """32 host games.TicTacToeEnv objects vs the device 'TicTacToe' env, 48 moves each, same planner seed: the replay's item count, every
    stored field and every priority are identical."""
    from muzero_amd import games, pipeline
    from muzero_amd.replay import PrioritizedReplay

    B, M = 32, 48
    net = build_mlp(mlp_case('tictactoe'))
    out = []
    for env in ('TicTacToe', [games.TicTacToeEnv() for _ in range(B)]):
        rp = PrioritizedReplay(4096, 0.0, 0.0, np.random.RandomState(0), device='cuda')
        steps = pipeline.run_self_play(_tictactoe_cfg(B), 0, net, torch.device('cuda', 0), env, rp, types.SimpleNamespace(value=0), _never(),
                                       max_moves=M)
        assert steps == B * M
        out.append(_replay_contents(rp))
    (n0, f0, p0), (n1, f1, p1) = out
    assert n0 == n1 and n0 > B  # (many games finished: TicTacToe lasts at most 10 moves)
    for f in FIELDS:
        assert np.array_equal(f0[f], f1[f]), f
    assert np.array_equal(p0, p1)


def test_tictactoe_host_envs_equal_device_env_into_queue():
    """The queue variant: the (Transition, priority) items the host assembles from the records are the same list, in the same order."""
    from muzero_amd import games, pipeline

    B, M = 32, 48
    net = build_mlp(mlp_case('tictactoe'))
    out = []
    for env in ('TicTacToe', lambda i: games.TicTacToeEnv()):
        q = queue.Queue()
        pipeline.run_self_play(_tictactoe_cfg(B), 0, net, torch.device('cuda', 0), env, q, types.SimpleNamespace(value=0), _never(), max_moves=M,
                               moves_per_drain=12)
        items = []
        while not q.empty():
            items.append(q.get())
        out.append(items)
    assert len(out[0]) == len(out[1]) > B
    for (t0, p0), (t1, p1) in zip(*out):
        assert p0 == p1
        for f in FIELDS:
            a, b = getattr(t0, f), getattr(t1, f)
            assert a.dtype == b.dtype and np.array_equal(a, b), f


def _planner(net, B, S, seed=5, **kw):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, num_simulations=S, seed=seed, **kw), 0)
    p.load_state_dict(net.state_dict())
    return p


def test_gomoku_conv_host_envs_equal_device_env_records():
    """Conv path: a 9 x 9 Gomoku board net, 16 envs, the board temperature schedule (temperature < 0: 1.0 for 30 moves, then 0.1),
    60 moves: every record of the host-stepped run (observation, action, reward, policy, root value, player, done) equals the device
    env's."""
    from muzero_amd import games
    from muzero_amd import planner as pl

    B, M, S = 16, 60, 8
    net = build_conv(conv_case('board9'))
    kw = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0))
    pd = _planner(net, B, S, **kw)
    pd.selfplay_reset(pl.ENV_GOMOKU)
    pd.selfplay_step(-1.0, M)
    dev = pd.selfplay_read(M)
    pd.close()

    ph = _planner(net, B, S, **kw)
    ph.selfplay_reset_external(frame_shape=(9, 9, 9), temp_switch_steps=30)
    envs = [games.GomokuEnv(board_size=9) for _ in range(B)]
    obs = [e.reset() for e in envs]
    for m in range(M):
        a = ph.external_act(np.stack(obs), np.stack([e.actions_mask for e in envs]), [e.current_player for e in envs],
                            [e.opponent_player for e in envs], -1.0)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for i, e in enumerate(envs):
            obs[i], rew[i], d, _ = e.step(int(a[i]))
            if d:
                obs[i] = e.reset()
            done[i] = d
        ph.external_commit(rew, done)
    host = ph.selfplay_read(M)
    c = ph.selfplay_counters()
    assert c['env_steps'] == B * M and c['simulations'] == B * M * S and c['episodes'] == int(host['done'].sum())
    ph.close()
    for k in REC:
        assert np.array_equal(dev[k], host[k]), k


class _CountingCartPoles:
    """CartPoleEnv objects with fixed per-env seeds (host stacking and device stacking see the same episodes)."""

    @staticmethod
    def make(B, seed0=100):
        from muzero_amd import games

        return [games.CartPoleEnv(seed=seed0 + i) for i in range(B)]


def test_cartpole_device_stacking_equals_host_stacking():
    """Vector frames: games.CartPoleEnv objects (StackFrameAndAction(4) inside PlayerIdAndActionMaskWrapper) with the same seeds,
    device_stack=True vs False, 40 envs x 120 moves (several episode resets): identical queue items, identical replay contents, and
    the recorded observations of the last moves equal."""
    from muzero_amd import pipeline
    from muzero_amd.config import make_classic_config
    from muzero_amd.replay import PrioritizedReplay

    B, M = 40, 120
    net = build_mlp(mlp_case('cartpole'))
    cfg = make_classic_config(use_tensorboard=False)
    cfg.num_envs, cfg.acc_seq_length, cfg.num_simulations = B, 20, 20
    res = {}
    for stack in (True, False):
        rp = PrioritizedReplay(8192, 0.0, 0.0, np.random.RandomState(0), device='cuda')
        pipeline.run_self_play(cfg, 0, net, torch.device('cuda', 0), _CountingCartPoles.make(B), rp, types.SimpleNamespace(value=0), _never(),
                               max_moves=M, device_stack=stack)
        q = queue.Queue()
        pipeline.run_self_play(cfg, 0, net, torch.device('cuda', 0), _CountingCartPoles.make(B), q, types.SimpleNamespace(value=0), _never(),
                               max_moves=M, device_stack=stack, env_threads=4 if stack else 1)
        items = []
        while not q.empty():
            items.append(q.get())
        res[stack] = (_replay_contents(rp), items)
    (r1, i1), (r0, i0) = res[True], res[False]
    assert r1[0] == r0[0] > B
    for f in FIELDS:
        assert np.array_equal(r1[1][f], r0[1][f]), f
    assert np.array_equal(r1[2], r0[2])
    assert len(i1) == len(i0) > B
    for (t1, p1), (t0, p0) in zip(i1, i0):
        assert p1 == p0 and all(np.array_equal(getattr(t1, f), getattr(t0, f)) for f in FIELDS)


class _FrameEnv:
    """A cheap seeded frame env: uint8 [1, 96, 96] frames drawn up front (every byte value occurs), random rewards, done every few steps."""

    num_actions = 6
    observation_shape = (1, 96, 96)

    def __init__(self, seed, n_frames=16):
        rs = np.random.RandomState(seed)
        self.frames = rs.randint(0, 256, size=(n_frames, 1, 96, 96)).astype(np.uint8)
        self.frames[0].reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
        self.rs = rs
        self.t = 0

    def reset(self, **kwargs):
        self.len = 2 + self.rs.randint(6)
        self.k = 0
        return self._frame()

    def _frame(self):
        self.t += 1
        return self.frames[(self.t - 1) % len(self.frames)]

    def step(self, action):
        self.k += 1
        return self._frame(), float(self.rs.randint(-2, 3)), self.k >= self.len, {}


def test_image_device_stacking_equals_host_scaled_stacking():
    """Image frames: the atari_s net ((4, 96, 96) = StackFrameAndAction(2) of [1, 96, 96]), uint8 frames scaled and stacked on the
    device, float32 frames (ScaledFloatFrame on the host) stacked on the device, and ScaledFloatFrame + StackFrameAndAction(is_obs_image=True)
    on the host: every record (observations included) equal over 24 moves of 8 envs with episode ends every few steps."""
    from muzero_amd import games
    from muzero_amd import planner as pl

    B, M, S = 8, 24, 4
    net = build_conv(conv_case('atari_s'))
    recs = []
    for mode in ('u8', 'f32', 'host'):
        p = _planner(net, B, S, discount=0.997)
        envs = [games.StackFrameAndAction(games.ScaledFloatFrame(_FrameEnv(40 + i)), 2, is_obs_image=True) for i in range(B)]
        if mode == 'u8':
            step = [e.env.env for e in envs]
            p.selfplay_reset_external(stack_history=2, is_obs_image=True, frame_shape=(1, 96, 96), frame_u8=True)
        elif mode == 'f32':
            step = [e.env for e in envs]
            p.selfplay_reset_external(stack_history=2, is_obs_image=True, frame_shape=(1, 96, 96))
        else:
            step = envs
            p.selfplay_reset_external(frame_shape=(4, 96, 96))
        obs = [e.reset() for e in step]
        for m in range(M):
            a = p.external_act(np.stack(obs), np.ones((B, 6), np.uint8), 1, 1, 1.0)
            rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
            for i, e in enumerate(step):
                obs[i], rew[i], d, _ = e.step(int(a[i]))
                if d:
                    obs[i] = e.reset()
                done[i] = d
            p.external_commit(rew, done)
        recs.append(p.selfplay_read(M))
        p.close()
    assert recs[0]['done'].sum() >= B
    for k in REC:
        assert np.array_equal(recs[0][k], recs[2][k]), k
        assert np.array_equal(recs[1][k], recs[2][k]), k
    # the scaling is numpy's float32 x / 255 for every byte value
    first = recs[0]['obs'][0, 0].reshape(4, 96, 96)[0].reshape(-1)[:256]
    assert np.array_equal(first, np.arange(256, dtype=np.uint8).astype(np.float32) / 255.0)


def test_external_errors():
    """Out-of-order calls return MZ_E_STATE, a stacked shape that is not the network's MZ_E_INVALID at reset, and an open trajectory
    longer than the record ring with a replay attached MZ_E_INVALID naming the env -- with the replay's count left at its last good value."""
    from muzero_amd import planner as pl
    from muzero_amd.replay import PrioritizedReplay

    B = 4
    net = build_mlp(mlp_case('cartpole'))
    p = _planner(net, B, 8, discount=0.997)
    with pytest.raises(pl.PlannerError, match='reset_external first'):
        p.external_commit(np.zeros(B), np.zeros(B))
    with pytest.raises(pl.PlannerError, match=r'error -1: .*stacked observation has 24 values.*20'):
        p.selfplay_reset_external(stack_history=4, frame_shape=(5,))
    p.selfplay_reset_external(stack_history=4, frame_shape=(4,))
    frames = np.zeros((B, 4), np.float32)
    with pytest.raises(pl.PlannerError, match=r'error -3: .*without an mz_selfplay_external_act'):
        p.external_commit(np.zeros(B), np.zeros(B))
    p.external_act(frames, np.ones((B, 2)), 1, 1, 1.0)
    with pytest.raises(pl.PlannerError, match=r'error -3: .*act twice'):
        p.external_act(frames, np.ones((B, 2)), 1, 1, 1.0)
    with pytest.raises(pl.PlannerError, match=r'error -3: .*mz_selfplay_step on host-stepped envs'):
        p.selfplay_step(1.0, 1)
    p.external_commit(np.ones(B), np.zeros(B))
    assert p.selfplay_counters()['env_steps'] == B

    # over-long episode: a record ring of 64 slots (the default; max_episode_steps 1 asks for no more), an episode of 65 moves
    cfg = types.SimpleNamespace(is_board_game=False, acc_seq_length=200, unroll_steps=3, td_steps=2, discount=0.997)
    rp = PrioritizedReplay(1024, 0.0, 0.0, np.random.RandomState(0), device='cuda')
    p.attach_replay(rp, cfg, obs_shape=(4, 5))
    p.selfplay_reset_external(stack_history=4, frame_shape=(4,), max_episode_steps=1)
    good = None
    with pytest.raises(pl.PlannerError, match=r'error -1: env 1: open trajectory of more than 64 moves'):
        for m in range(70):
            p.external_act(frames, np.ones((B, 2)), 1, 1, 1.0)
            done = np.array([1, 0, 1, 1], np.uint8)  # env 1 never finishes
            good = rp.num_added
            p.external_commit(np.ones(B), done)
    assert m == 64 and good > 0
    assert rp.num_added == good
    with pytest.raises(pl.PlannerError, match=r'error -3: .*over-long'):
        p.external_act(frames, np.ones((B, 2)), 1, 1, 1.0)
    p.detach_replay()
    assert rp.num_added == good
    p.close()
