#!/usr/bin/env python3
"""Env-steps per second of self-play on host-stepped environments (Planner.external_act / external_commit, the loop of
pipeline.run_self_play over env objects) against the device environments, at the BASELINE.json shapes:
  c5 : 256 host games.GomokuEnv(15) vs the device 'Gomoku' env (C5 net, 200 simulations, board temperature schedule);
  c4 : 512 envs of a cheap host frame env (pre-drawn uint8 [1, 96, 96] frames) with StackFrameAndAction(4) on the device vs on the
       host (ScaledFloatFrame + StackFrameAndAction, float32 observations uploaded) vs the device 'Synthetic-Atari' env (C4 net, 50 sims);
  c2 : 4096 host games.CartPoleEnv (stacking on the device) vs the device CartPole env, reported only (Python stepping dominates).
Every figure is host-inclusive wall time over `moves` lock-step moves after `warm` untimed ones; one JSON line per leg.  Run it under
`rocprofv3 --kernel-trace --stats` for the per-kernel times (k_ext_ingest's time per move and bytes / time).
    python tools/hostenv_bench.py [--legs c5,c4,c2] [--moves N] [--warm N]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import numpy as np  # noqa: E402

from helpers import build_conv, build_mlp, mlp_case  # noqa: E402
from muzero_amd import games  # noqa: E402
from muzero_amd import planner as pl  # noqa: E402

C4 = ('c4', 'atari', (8, 96, 96), 6, 8, 128, 61, 61, 41)  # bench.py CONV_WORKLOADS
C5 = ('c5', 'board', (9, 15, 15), 226, 8, 128, 1, 1, 42)


class FrameEnv:
    """Pre-drawn uint8 [1, 96, 96] frames, reward 0, an episode end every 1000 steps (the Synthetic-Atari env's shape)."""

    num_actions = 6
    observation_shape = (1, 96, 96)

    def __init__(self, seed, n_frames=8):
        self.frames = np.random.RandomState(seed).randint(0, 256, size=(n_frames, 1, 96, 96)).astype(np.uint8)
        self.t = self.k = 0

    def reset(self, **kwargs):
        self.k = 0
        return self._frame()

    def _frame(self):
        self.t += 1
        return self.frames[self.t % len(self.frames)]

    def step(self, action):
        self.k += 1
        return self._frame(), 0.0, self.k >= 1000, {}


def planner(net, B, S, **kw):
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=1000, num_simulations=S, root_exploration_eps=0.25, **kw), 0)
    p.load_state_dict(net.state_dict())
    return p


def device_rate(net, B, S, kind, T, moves, warm, **kw):
    p = planner(net, B, S, **kw)
    p.selfplay_reset(kind)
    p.selfplay_step(T, warm)
    p.synchronize()
    t0 = time.perf_counter()
    p.selfplay_step(T, moves)
    p.synchronize()
    dt = time.perf_counter() - t0
    p.close()
    return B * moves / dt, dt / moves


def host_rate(net, B, S, envs, T, moves, warm, stack=0, image=False, frame_shape=None, u8=False, temp_switch=0, **kw):
    """The pipeline's host loop: gather mask / players, one external_act, env.step on the host (reset on done), one external_commit.
    Returns (env steps / s, s / move, host seconds / move spent outside the planner calls)."""
    p = planner(net, B, S, **kw)
    p.selfplay_reset_external(stack_history=stack, is_obs_image=image, frame_shape=frame_shape, frame_u8=u8, temp_switch_steps=temp_switch)
    frames = [np.asarray(e.reset()) for e in envs]
    dt = np.uint8 if u8 else np.float32
    A = p.A
    ones = np.ones((B, A), np.uint8)
    rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
    t0 = host = 0.0
    for m in range(warm + moves):
        if m == warm:
            t0, host = time.perf_counter(), 0.0
        h0 = time.perf_counter()
        mask = np.stack([e.actions_mask for e in envs]).astype(np.uint8) if hasattr(envs[0], 'actions_mask') else ones
        cur = np.array([getattr(e, 'current_player', 1) for e in envs], np.int32)
        opp = np.array([getattr(e, 'opponent_player', 1) for e in envs], np.int32)
        x = np.stack(frames).astype(dt, copy=False)
        h1 = time.perf_counter()
        a = p.external_act(x, mask, cur, opp, T)
        h2 = time.perf_counter()
        for i, e in enumerate(envs):
            o, r, d, _ = e.step(int(a[i]))
            if d:
                o = e.reset()
            frames[i], rew[i], done[i] = o, r, d
        h3 = time.perf_counter()
        p.external_commit(rew, done)
        host += (h1 - h0) + (h3 - h2)
    p.synchronize()
    wall = time.perf_counter() - t0
    p.close()
    return B * moves / wall, wall / moves, host / moves


def emit(rec):
    print(json.dumps(rec), flush=True)


def leg_c5(moves, warm):
    net, B, S = build_conv(C5), 256, 200
    kw = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.03)
    dev, dev_mv = device_rate(net, B, S, pl.ENV_GOMOKU, -1.0, moves, warm, **kw)
    envs = [games.GomokuEnv(board_size=15) for _ in range(B)]
    host, host_mv, host_py = host_rate(net, B, S, envs, -1.0, moves, warm, frame_shape=(9, 15, 15), temp_switch=30, **kw)
    emit({'leg': 'c5', 'what': '256 host GomokuEnv(15) vs device Gomoku, C5 net, 200 sims', 'moves': moves,
          'device_env_steps_per_s': dev, 'device_ms_per_move': dev_mv * 1e3, 'host_env_steps_per_s': host, 'host_ms_per_move': host_mv * 1e3,
          'host_python_ms_per_move': host_py * 1e3, 'host_over_device': host / dev})


def leg_c4(moves, warm):
    net, B, S = build_conv(C4), 512, 50
    kw = dict(discount=0.997, root_dirichlet_alpha=0.25)
    dev, dev_mv = device_rate(net, B, S, pl.ENV_SYNTHETIC, 1.0, moves, warm, **kw)
    envs = [FrameEnv(i) for i in range(B)]
    ds, ds_mv, ds_py = host_rate(net, B, S, envs, 1.0, moves, warm, stack=4, image=True, frame_shape=(1, 96, 96), u8=True, **kw)
    envs = [games.StackFrameAndAction(games.ScaledFloatFrame(FrameEnv(i)), 4, is_obs_image=True) for i in range(B)]
    hs, hs_mv, hs_py = host_rate(net, B, S, envs, 1.0, moves, warm, frame_shape=(8, 96, 96), **kw)
    emit({'leg': 'c4', 'what': '512 host uint8 frame envs, C4 net, 50 sims: device stacking vs host stacking vs device Synthetic-Atari', 'moves': moves,
          'synthetic_env_steps_per_s': dev, 'synthetic_ms_per_move': dev_mv * 1e3,
          'device_stack_env_steps_per_s': ds, 'device_stack_ms_per_move': ds_mv * 1e3, 'device_stack_python_ms_per_move': ds_py * 1e3,
          'host_stack_env_steps_per_s': hs, 'host_stack_ms_per_move': hs_mv * 1e3, 'host_stack_python_ms_per_move': hs_py * 1e3,
          'device_stack_over_synthetic': ds / dev, 'device_stack_over_host_stack': ds / hs,
          'upload_bytes_per_move': {'device_stack': B * 96 * 96, 'host_stack': B * 8 * 96 * 96 * 4}})


def leg_c2(moves, warm):
    net, B, S = build_mlp(mlp_case('cartpole')), 4096, 50
    kw = dict(discount=0.997, root_dirichlet_alpha=0.25)
    dev, dev_mv = device_rate(net, B, S, pl.ENV_CARTPOLE, 1.0, moves, warm, **kw)
    envs = [games.CartPoleEnv(seed=i) for i in range(B)]
    base = [e.env.env for e in envs]
    host, host_mv, host_py = host_rate(net, B, S, base, 1.0, moves, warm, stack=4, frame_shape=(4,), **kw)
    emit({'leg': 'c2', 'what': '4096 host CartPoleEnv (device stacking) vs device CartPole, 50 sims (reported only: Python stepping dominates)',
          'moves': moves, 'device_env_steps_per_s': dev, 'device_ms_per_move': dev_mv * 1e3, 'host_env_steps_per_s': host,
          'host_ms_per_move': host_mv * 1e3, 'host_python_ms_per_move': host_py * 1e3})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='c5,c4,c2')
    ap.add_argument('--moves', type=int, default=0, help='timed moves per run (default per leg: c5 4, c4 12, c2 20)')
    ap.add_argument('--warm', type=int, default=2)
    a = ap.parse_args()
    legs = {'c5': (leg_c5, 4), 'c4': (leg_c4, 12), 'c2': (leg_c2, 20)}
    for name in a.legs.split(','):
        fn, n = legs[name]
        fn(a.moves or n, a.warm)


if __name__ == '__main__':
    main()
