"""Timing of the arena (Planner.arena_*) on the full-size Gomoku net, beside its two baselines.

    python tools/arena_bench.py [--board 15] [--games 256] [--sims 200] [--plies 12] [--host-games 1] [--host-plies 12] [--out FILE]

Prints one JSON line (and writes it to --out):
  arena        : `--games` games of the C5-shaped net (8 blocks, 128 planes) against a second seed, `--plies` plies timed after 2
                 warm-up plies: ms per ply, and per game scaled to the board's point count (the cap of a game's length)
  search_pair  : two mz_planner_search calls of batch games / 2, deterministic, on the same handles and box: what a ply costs without
                 the arena's own kernels and stream ordering (it includes the calls' uploads and downloads, which the arena does not have)
  host_loop    : the host evaluator loop (mcts.uct_search at batch 1 on games.GomokuEnv, deterministic), timed for `--host-plies`
                 plies of `--host-games` games and scaled to the same game and ply count.  The baseline; never the arena itself.
`--trace` runs only the arena plies (for a kernel-trace statistics run around this script)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--games', type=int, default=256)
    ap.add_argument('--sims', type=int, default=200)
    ap.add_argument('--plies', type=int, default=12)
    ap.add_argument('--host-games', type=int, default=1)
    ap.add_argument('--host-plies', type=int, default=12)
    ap.add_argument('--blocks', type=int, default=8)
    ap.add_argument('--planes', type=int, default=128)
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()

    import torch
    from muzero_amd import mcts, network, planner as pl
    from muzero_amd.config import make_gomoku_config
    from muzero_amd.games import GomokuEnv

    N, B, A = args.board, args.games, args.board ** 2 + 1
    cfg = make_gomoku_config(use_tensorboard=False)
    cfg.num_simulations = args.sims
    nets = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        net = network.MuZeroBoardGameNet((9, N, N), A, args.blocks, args.planes)
        net.eval()
        nets.append(net)
    p = pl.Planner(pl.make_mz_config(nets[0].planner_spec(), cfg, num_envs=B, seed=11), 0)
    q = pl.Planner(pl.make_mz_config(nets[1].planner_spec(), cfg, num_envs=B, seed=12), 0)
    p.load_state_dict(nets[0].state_dict())
    q.load_state_dict(nets[1].state_dict())
    p.arena_reset(pl.ENV_GOMOKU, q, opening_plies=2)
    p.arena_step(2)
    p.synchronize()
    t0 = time.perf_counter()
    p.arena_step(args.plies)
    live = p.arena_result()['live']  # (drains both planners' streams)
    ply_ms = (time.perf_counter() - t0) * 1e3 / args.plies
    out = dict(board=N, games=B, sims=args.sims, blocks=args.blocks, planes=args.planes,
               arena=dict(plies_timed=args.plies, ms_per_ply=ply_ms, live_after=live, s_per_game_at_cap=ply_ms * N * N / 1e3,
                          s_per_match_at_cap=ply_ms * N * N / 1e3))
    if not args.trace:
        rec = p.arena_read_ply()
        half = B // 2
        obs, mask = rec['obs'][:half], np.ones((half, A), np.uint8)
        for h in (p, q):
            h.search(obs, mask, 1, 2, 1.0, deterministic=True)
        t0 = time.perf_counter()
        reps = 3
        for _ in range(reps):
            for h in (p, q):
                h.search(obs, mask, 1, 2, 1.0, deterministic=True)
        pair_ms = (time.perf_counter() - t0) * 1e3 / reps
        out['search_pair'] = dict(batch=half, ms_per_pair=pair_ms, arena_own_ms_per_ply=ply_ms - pair_ms)
        p.close()
        q.close()
        dev = torch.device('cuda', 0)
        cfg.num_envs = 1
        env = GomokuEnv(N)
        plies, t_host = 0, 0.0
        for g in range(args.host_games):
            obs_h, done = env.reset(), False
            for net in nets:  # warm-up: each network's planner is created at its first search
                mcts.uct_search(obs_h, net, dev, cfg, 0.1, env.actions_mask, env.current_player, env.opponent_player, True)
            t0 = time.perf_counter()
            for _ in range(args.host_plies):
                net = nets[0] if env.current_player == env.black_player_id else nets[1]
                a, *_ = mcts.uct_search(obs_h, net, dev, cfg, 0.1, env.actions_mask, env.current_player, env.opponent_player, True)
                obs_h, _, done, _ = env.step(a)
                plies += 1
                if done:
                    break
            t_host += time.perf_counter() - t0
        host_ply_ms = t_host * 1e3 / max(plies, 1)
        out['host_loop'] = dict(plies_timed=plies, ms_per_ply_one_game=host_ply_ms, s_per_match_at_cap=host_ply_ms * N * N * B / 1e3,
                                speedup_per_ply=host_ply_ms * B / ply_ms)
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
