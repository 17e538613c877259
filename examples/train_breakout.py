#!/usr/bin/env python3
"""End-to-end MuZero with `MuZeroAtariNet` on Breakout, the device image game that pays rewards during the episode: device Breakout
self-play (96 x 96 uint8 frames rendered on the device, stacked 4 deep, kept in a compact `frames_u8` record ring) -> device epilogue into a
`frames_u8` HBM replay -> `DeviceSampler` -> the Atari `HipLearner` step -> weights repacked into the planner on the GPU.  The run uses
what Catch cannot: the reward head sees nonzero targets, the value target is a bootstrapped 10-step return with discount 0.997, and
episodes are cut by a move cap.  One process, one GPU, event order, as `train_catch.py` (whose flags these are).

    python examples/train_breakout.py --train-steps 2000 --envs 256

Evaluation: `--eval-envs` host `games.BreakoutEnv` objects play one lock-step batch with deterministic `Planner.search`; the start codes
cover every ball column and both directions equally often.  One JSON line per evaluation with the mean return (bricks broken), its
standard error and the mean episode length.  `--arena-eval N` (N > 0) plays the evaluations on the device instead: `pipeline.play_match` on
the Breakout arena, N games rounded up to a multiple of the 2 * cols start codes, nothing crossing PCIe.  `--random-return R` gives the
uniformly random policy's mean return to compare the last evaluation with (default 0.18, 2 000 host episodes on the 12 x 12 grid)."""
import argparse
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
    ap.add_argument('--train-steps', type=int, default=2000)
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--moves-per-iter', type=int, default=4)
    ap.add_argument('--updates-per-iter', type=int, default=8)
    ap.add_argument('--batch-size', type=int, default=128)
    ap.add_argument('--min-replay', type=int, default=4000)
    ap.add_argument('--replay-size', type=int, default=50000)
    ap.add_argument('--simulations', type=int, default=25)
    ap.add_argument('--planes', type=int, default=32)
    ap.add_argument('--blocks', type=int, default=2)
    ap.add_argument('--lr', type=float, default=0.002)
    ap.add_argument('--report-every', type=int, default=200)
    ap.add_argument('--eval-every', type=int, default=500, help='evaluate every N training steps (and at the end); 0: only at the end')
    ap.add_argument('--eval-envs', type=int, default=96, help='evaluation episodes, rounded up to a multiple of the 24 start codes')
    ap.add_argument('--arena-eval', type=int, default=0, help='N > 0: evaluate with N games (rounded up to a multiple of the 24 start codes) on the device '
                    'Breakout arena instead of the --eval-envs host envs')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--random-return', type=float, default=0.18, help='the random policy\'s mean return, for the final comparison')
    ap.add_argument('--random-se', type=float, default=0.01, help='its standard error')
    ap.add_argument('--tower-precision', choices=('f32', 'bf16x3'), default='f32', help='planner and learner: the fused residual towers')
    ap.add_argument('--stage-precision', choices=('f32', 'bf16x3'), default='f32', help='learner: the tile path\'s stride-1 convs')
    ap.add_argument('--record-format', choices=('f32', 'frames_u8'), default='frames_u8', help='the self-play record ring')
    ap.add_argument('--out', default='')
    args = ap.parse_args()

    from muzero_amd import games, learner
    from muzero_amd import planner as pl
    from muzero_amd.config import make_breakout_config
    from muzero_amd.network import MuZeroAtariNet
    from muzero_amd.replay import PrioritizedReplay

    torch.manual_seed(args.seed)
    dev = torch.device('cuda', 0)
    cfg = make_breakout_config(num_training_steps=args.train_steps, batch_size=args.batch_size, min_replay_size=args.min_replay)
    cfg.num_envs, cfg.num_simulations, cfg.num_planes, cfg.num_res_blocks, cfg.lr_init = args.envs, args.simulations, args.planes, args.blocks, args.lr
    S, rows, cols, K, cap = cfg.stack_history, cfg.rows, cfg.cols, cfg.brick_rows, cfg.max_moves
    H, W = cfg.input_shape[1:]
    net = MuZeroAtariNet(cfg.input_shape, cfg.num_actions, cfg.num_res_blocks, cfg.num_planes, cfg.value_support_size, cfg.reward_support_size).to(dev)
    hl = learner.make_hip_learner(cfg, net, dev, tower_precision=args.tower_precision, stage_precision=args.stage_precision)
    replay = PrioritizedReplay(args.replay_size, 0.0, 0.0, np.random.RandomState(args.seed), device='cuda', state_format='frames_u8',
                               frame_spec=(S, 1, H, W, cfg.num_actions))

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), cfg, num_envs=args.envs, seed=args.seed), 0, tower_precision=args.tower_precision)
    net.eval()
    p.reload(hl.planner_weights())
    p.attach_replay(replay, cfg, obs_shape=cfg.input_shape)
    p.selfplay_reset_breakout(rows, cols, K, cap, record_format=args.record_format)
    sampler = replay.device_sampler(seed=args.seed)

    arena = args.arena_eval > 0
    n_eval = -(-(args.arena_eval if arena else args.eval_envs) // (2 * cols)) * (2 * cols)
    pe = None if arena else pl.Planner(pl.make_mz_config(net.planner_spec(), cfg, num_envs=n_eval, seed=args.seed + 1), 0, tower_precision=args.tower_precision)
    random_return = args.random_return

    def make_env():
        return games.BreakoutEnv(rows, cols, H // rows, W // cols, brick_rows=K, max_moves=cap)

    def report(rets, lens):
        return dict(eval_mean_return=float(rets.mean()), eval_standard_error=float(rets.std(ddof=1) / np.sqrt(n_eval)),
                    eval_mean_length=float(np.mean(lens)), eval_episodes=n_eval, random_policy_return=random_return)

    def evaluate_arena():
        """n_eval games in lock-step on the device Breakout arena, start code i % (2 cols): the same greedy search, no host env."""
        import types

        from muzero_amd import pipeline

        cfg.planner_seed, cfg.tower_precision = args.seed + 1, args.tower_precision
        weights = types.SimpleNamespace(planner_spec=net.planner_spec, state_dict=hl.planner_weights)  # the learner's weights, still on the GPU
        m = pipeline.play_match(cfg, weights, None, dev, make_env(), n_eval, tag='train_breakout')
        return report(m.ret, m.length)

    def evaluate():
        """n_eval host envs in one lock-step batch, start code i % (2 cols): greedy search, no noise; a finished env's slot repeats its last
        observation and is no longer stepped."""
        net.eval()
        if arena:
            return evaluate_arena()
        pe.reload(hl.planner_weights())
        envs = [games.make_breakout_env(rows, cols, H // rows, W // cols, stack_history=S, brick_rows=K, max_moves=cap) for _ in range(n_eval)]
        obs = [e.reset(start_code=i % (2 * cols)) for i, e in enumerate(envs)]
        mask = np.ones((n_eval, cfg.num_actions), bool)
        rets, lens, live = np.zeros(n_eval), np.zeros(n_eval, int), np.ones(n_eval, bool)
        while live.any():
            act = pe.search(np.stack(obs), mask, 1, 1, 0.0, deterministic=True)['action']
            for i in np.flatnonzero(live):
                obs[i], r, d, _ = envs[i].step(int(act[i]))
                rets[i] += r
                lens[i] += 1
                live[i] = not d
        return report(rets, lens)

    steps, t0, last = 0, time.time(), dict(episodes=0)
    log, evals = [], []
    ev = dict(train_steps=0, seconds=0.0, **evaluate())
    evals.append(ev)
    print(json.dumps(ev), flush=True)
    while steps < args.train_steps:
        T = float(cfg.visit_softmax_temperature_fn(0, steps))
        p.selfplay_step(T, args.moves_per_iter)
        p.synchronize()  # event order: the moves above are in the replay before anything is drawn from it
        if replay.size < cfg.min_replay_size:
            continue
        net.train()
        for _ in range(args.updates_per_iter):
            idx_t, w_t, ring = sampler.sample(cfg.batch_size)  # draw, gather, update: all on the device
            loss, prio = hl.step(ring, idx_t, w_t, cfg.batch_size)
            steps += 1
            if steps % args.report_every == 0:
                c = p.selfplay_counters()
                rec = dict(train_steps=steps, env_steps=int(c['env_steps']), episodes=int(c['episodes']), loss=float(loss), replay=replay.size,
                           seconds=round(time.time() - t0, 1))
                log.append(rec)
                print(json.dumps(rec), flush=True)
        net.eval()
        p.reload(hl.planner_weights())  # actor <- learner, packed on the GPU
        if args.eval_every and steps < args.train_steps and steps // args.eval_every > (steps - args.updates_per_iter) // args.eval_every:
            ev = dict(train_steps=steps, seconds=round(time.time() - t0, 1), **evaluate())
            evals.append(ev)
            print(json.dumps(ev), flush=True)
    ev = dict(train_steps=steps, seconds=round(time.time() - t0, 1), **evaluate())
    evals.append(ev)
    print(json.dumps(ev), flush=True)
    learned = ev['eval_mean_return'] - random_return > 3 * float(np.hypot(ev['eval_standard_error'], args.random_se))
    idx_t, _, ring = sampler.sample(cfg.batch_size)  # one more batch: how much the reward head has to learn from
    targets = ring['reward'][idx_t]
    nonzero = dict(batch=float((targets != 0).float().mean()), replay=float((ring['reward'][:replay.size] != 0).float().mean()))
    summary = dict(final=ev, learned=bool(learned), reward_targets_nonzero_fraction=nonzero, record_info=p.record_info(), env_steps=int(p.selfplay_counters()['env_steps']))
    print(json.dumps(summary), flush=True)
    if args.out:
        json.dump(dict(args=vars(args), log=log, evals=evals, summary=summary), open(args.out, 'w'), indent=1)
    p.close()
    if pe is not None:
        pe.close()


if __name__ == '__main__':
    main()
