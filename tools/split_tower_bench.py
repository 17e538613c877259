#!/usr/bin/env python3
"""The split-bf16 fused residual tower (csrc/mz_tower_split.h) against the float32 paths.  Seeded random weights; every leg is a fresh child
process; legs alternate between the arms, at least two per arm.

    python tools/split_tower_bench.py [--legs 2] [--moves 2] [--warm 1] [--out profiles/split_tower] [--parent-tree PATH]

  c4_move      Atari net 128 planes x 8 blocks, 8 x 96 x 96, 512 envs x 50 simulations on the synthetic env: ms per self-play move with
               tower_precision f32 and bf16x3; --parent-tree PATH adds the float32 move of a built checkout of the parent commit (its package
               and library, in a child process of its own)
  tower        ONE tower launch, 16 convs x 128 planes on 512 6 x 6 images, k_res_tower against k_res_tower_bf16x3, between two HIP
               events on the planner's stream (Planner.debug_res_tower(timed=True)), best of 10 after a warm-up launch
  board_split  board net 9 x 9, 64 planes x 4 blocks, 256 envs x 50 simulations, conv_precision bf16x3 on the device Gomoku env: the fused
               split tower against MZ_TOWER=0 (one launch per conv)
Writes <out>/split_tower_bench.json."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

C4 = ('c4', 'atari', (8, 96, 96), 4, 8, 128, 61, 61, 42)
B9 = ('b9', 'board', (9, 9, 9), 82, 4, 64, 1, 1, 42)
ARMS = {
    'c4_move': ['f32', 'bf16x3'],
    'tower': ['f32', 'bf16x3'],
    'board_split': ['fused', 'per_conv'],
}


def _move_ms(p, pl, env, temp, moves, warm):
    import torch

    p.selfplay_reset(env)
    if warm:
        p.selfplay_step(temp, warm)
    p.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.selfplay_step(temp, moves)
    p.synchronize()
    return (time.perf_counter() - t0) / moves * 1e3


def child(workload, arm, moves, warm):
    import numpy as np
    from helpers import build_conv
    from muzero_amd import planner as pl

    res = dict(workload=workload, arm=arm)
    if workload == 'c4_move':
        net = build_conv(C4)
        cfg = pl.make_mz_config(net.planner_spec(), None, num_envs=512, seed=1000, num_simulations=50, discount=0.997, root_dirichlet_alpha=0.25,
                                root_exploration_eps=0.25)
        p = pl.Planner(cfg, 0, tower_precision='bf16x3') if arm == 'bf16x3' else pl.Planner(cfg, 0)  # (a parent build has no tower_precision)
        p.load_state_dict(net.state_dict())
        res.update(ms_per_move=_move_ms(p, pl, pl.ENV_SYNTHETIC, 1.0, moves, warm), envs=512, sims=50)
    elif workload == 'board_split':
        net = build_conv(B9)
        p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=256, seed=1000, num_simulations=50, discount=1.0, is_board_game=True,
                                         known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.03, root_exploration_eps=0.25, conv_precision='bf16x3'), 0)
        p.load_state_dict(net.state_dict())
        res.update(ms_per_move=_move_ms(p, pl, pl.ENV_GOMOKU, -1.0, moves, warm), envs=256, sims=50)
    else:
        net = build_conv(('t', 'atari', (8, 96, 96), 4, 1, 16, 61, 61, 1))
        p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=4), 0, tower_precision=arm)
        rs = np.random.RandomState(1)
        x = rs.uniform(0, 1, (512, 128, 6, 6)).astype(np.float32)
        w = (rs.randn(16, 128, 128, 3, 3) * np.sqrt(2.0 / 1152)).astype(np.float32)
        b = (rs.randn(16, 128) * 0.1).astype(np.float32)
        p.debug_res_tower(x, w, b)
        ts = []
        for _ in range(10):
            _, name, ms = p.debug_res_tower(x, w, b, timed=True)
            ts.append(ms)
        res.update(build=name, tower_ms=min(ts), tower_ms_median=sorted(ts)[len(ts) // 2], convs=16, images=512)
    res['describe'] = p.describe()
    p.close()
    print(json.dumps(res), flush=True)


def run_child(workload, arm, moves, warm, parent_lib=''):
    env = dict(os.environ)
    if workload == 'board_split' and arm == 'per_conv':
        env['MZ_TOWER'] = '0'
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--workload', workload, '--arm', arm, '--moves', str(moves), '--warm', str(warm)]
    if arm == 'f32-parent':
        cmd += ['--tree', parent_lib]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f'{workload} / {arm} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--workload', default='')
    ap.add_argument('--arm', default='f32')
    ap.add_argument('--tree', default='', help='(child) import muzero_amd and the test helpers from this checkout instead')
    ap.add_argument('--parent-tree', default='', help='a built checkout of the parent commit: adds the arm f32-parent to c4_move')
    ap.add_argument('--legs', type=int, default=2)
    ap.add_argument('--moves', type=int, default=2)
    ap.add_argument('--warm', type=int, default=1)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.child:
        if a.tree:
            sys.path[:0] = [os.path.abspath(a.tree), os.path.join(os.path.abspath(a.tree), 'tests')]
        return child(a.workload, 'f32' if a.arm == 'f32-parent' else a.arm, a.moves, a.warm)
    arms = {k: list(v) for k, v in ARMS.items()}
    if a.parent_tree:
        arms['c4_move'].append('f32-parent')
    summary = {}
    for w in ([a.workload] if a.workload else list(arms)):
        legs = []
        for _ in range(max(a.legs, 2)):
            for arm in arms[w]:
                leg = run_child(w, arm, a.moves, a.warm, a.parent_tree)
                leg['arm'] = arm
                legs.append(leg)
                print(json.dumps(leg), flush=True)
        key = 'tower_ms' if w == 'tower' else 'ms_per_move'
        s = dict(legs=legs)
        for arm in arms[w]:
            v = sorted(leg[key] for leg in legs if leg['arm'] == arm)
            s[arm] = {key + '_min': v[0], key + '_max': v[-1]}
        first, second = arms[w][0], arms[w][1]
        s[f'{second}_over_{first}' if w == 'board_split' else f'speedup_{second}_over_{first}'] = \
            s[second][key + '_min'] / s[first][key + '_min'] if w == 'board_split' else s[first][key + '_min'] / s[second][key + '_min']
        summary[w] = s
        print(json.dumps({w: {k: v for k, v in s.items() if k != 'legs'}}), flush=True)
    if a.out:
        path = a.out if a.out.endswith('.json') else os.path.join(a.out, 'split_tower_bench.json')
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            json.dump(summary, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
