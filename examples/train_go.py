#!/usr/bin/env python3
"""End-to-end MuZero on Go (7 x 7 by default: 51 actions -- 49 points, pass, resign; komi 7.5) with a small board conv net, on the pattern of
examples/train_othello.py: device self-play on the device Go env (`Planner.selfplay_reset_go`, csrc/mz_go.h) -> device epilogue -> HBM
replay ring (float32 states, or `--replay-state int8`: one exact byte per element of the 0 / 1 planes) -> batch indices drawn on the
device -> the hand-written conv learner (`hip_learner.HipLearner`) -> `Planner.reload`.  Nothing of a trajectory leaves the GPU.

`--resign` (default off) makes the resignation a legal action (`allow_resign`).  profiles/go/learning.json and learning_resign.json hold
this script's runs either way: with these defaults NEITHER learns to beat the uniformly random opponent in 1 500 updates (README).  `--komi2`
is twice the komi; 15 (7.5 points) is the default: a half-integer komi leaves no draws.  Uniformly random play against itself on 7 x 7
then gives black 33 % and white 67 % (profiles/go/random_policy.json); the arena balances colours, so the baseline against the random
opponent is 50 %.  `--max-plies` ends a game by the count (0: 2 * rows * cols).

Evaluation is the device arena (`pipeline.play_match(..., 'Go', N)`): `--arena-eval N` plays N games (even; colours balanced, two random
opening plies per pair) against the uniformly random opponent, which may pass and never resigns, and N against the previous
checkpoint, before training and every `--report-every` updates.

    python examples/train_go.py --train-steps 1500 --envs 256 --arena-eval 256 [--resign] [--replay-state int8]"""
import argparse
import copy
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--train-steps', type=int, default=1500)
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--simulations', type=int, default=32)
    ap.add_argument('--planes', type=int, default=32)
    ap.add_argument('--blocks', type=int, default=2)
    ap.add_argument('--rows', type=int, default=7)
    ap.add_argument('--cols', type=int, default=7)
    ap.add_argument('--komi2', type=int, default=15, help='twice the komi')
    ap.add_argument('--max-plies', type=int, default=0, help='the ply that ends a game by the count (0: 2 * rows * cols)')
    ap.add_argument('--resign', action='store_true', help='make the resignation a legal action (allow_resign)')
    ap.add_argument('--moves-per-iter', type=int, default=8)
    ap.add_argument('--updates-per-iter', type=int, default=16)
    ap.add_argument('--min-replay', type=int, default=4000)
    ap.add_argument('--report-every', type=int, default=250)
    ap.add_argument('--arena-eval', type=int, default=256, metavar='N', help='N arena games (even) against the random opponent and against the previous checkpoint; 0: off')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--replay-state', choices=['f32', 'int8'], default='f32', help='how the replay stores states: float32, or one exact byte per element')
    ap.add_argument('--out', default='')
    args = ap.parse_args()

    from muzero_amd import learner
    from muzero_amd import planner as pl
    from muzero_amd.config import make_go_config
    from muzero_amd.network import MuZeroBoardGameNet
    from muzero_amd.pipeline import play_match
    from muzero_amd.replay import PrioritizedReplay

    torch.manual_seed(args.seed)
    dev = torch.device('cuda', 0)
    cfg = make_go_config(num_training_steps=args.train_steps, batch_size=128, min_replay_size=args.min_replay, rows=args.rows, cols=args.cols,
                         komi2=args.komi2, max_plies=args.max_plies, allow_resign=args.resign, num_simulations=args.simulations)
    cfg.num_envs, cfg.num_planes, cfg.num_res_blocks, cfg.planner_seed = args.envs, args.planes, args.blocks, args.seed
    net = MuZeroBoardGameNet(cfg.input_shape, cfg.num_actions, cfg.num_res_blocks, cfg.num_planes).to(dev)
    hip = learner.make_hip_learner(cfg, net, dev)  # the module's parameters and BatchNorm buffers become views of the learner's flat vectors
    replay = PrioritizedReplay(40000, 0.0, 0.0, np.random.RandomState(args.seed), device='cuda', state_format=None if args.replay_state == 'f32' else args.replay_state)
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), cfg, num_envs=args.envs, seed=args.seed), 0)
    net.eval()
    p.reload(hip.planner_weights())
    p.attach_replay(replay, cfg, obs_shape=cfg.input_shape)
    p.selfplay_reset_go(cfg.komi2, cfg.max_plies, cfg.allow_resign, cfg.temp_switch_steps)
    sampler = replay.device_sampler(seed=args.seed)
    previous = copy.deepcopy(net)  # the checkpoint of the last report: the second arena opponent

    def arena():
        if args.arena_eval <= 0:
            return {}
        out = {}
        for name, opponent in (('random', 'random'), ('previous', previous)):
            m = play_match(cfg, net, opponent, dev, 'Go', args.arena_eval, opening_plies=2)  # (the rules come off cfg)
            out['vs_' + name] = dict(games=m.num_games, win=m.wins, draw=m.draws, loss=m.losses, mean_length=float(m.length.mean()), **m.by_colour())
        previous.load_state_dict(net.state_dict())
        return out

    t0 = time.time()
    log = [dict(train_steps=0, seconds=0.0, **arena())]
    print(json.dumps(log[0]), flush=True)
    steps = 0
    while steps < args.train_steps:
        p.selfplay_step(-1.0, args.moves_per_iter)  # the game's own temperature schedule, per env
        p.synchronize()  # the moves above are committed to the ring before a batch is drawn
        if replay.size < cfg.min_replay_size:
            continue
        net.train()
        for _ in range(args.updates_per_iter):
            idx_t, w_t, ring = sampler.sample(cfg.batch_size)
            loss, _ = hip.step(ring, idx_t, w_t, cfg.batch_size)
            steps += 1
            if steps % args.report_every == 0:
                net.eval()
                c = p.selfplay_counters()
                rec = dict(train_steps=steps, loss=float(loss), seconds=round(time.time() - t0, 1), env_steps=int(c['env_steps']), episodes=int(c['episodes']),
                           mean_episode_length=c['episode_steps'] / max(c['episodes'], 1), **arena())
                net.train()
                log.append(rec)
                print(json.dumps(rec), flush=True)
            if steps >= args.train_steps:
                break
        net.eval()
        p.reload(hip.planner_weights())
    if args.out:
        json.dump(dict(args=vars(args), log=log), open(args.out, 'w'), indent=1)
    p.close()


if __name__ == '__main__':
    main()
