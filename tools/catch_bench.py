#!/usr/bin/env python3
"""Measurements of the device Catch env (MZ_ENV_CATCH); each mode writes one JSON file under profiles/catch/ (or --out).

    python tools/catch_bench.py move      [--steps 8 --warmup 2]     # (a) one self-play move at C4 shape, three ways, same process
    python tools/catch_bench.py trace                                # (a) the step / render kernels' own time from a kernel trace
    python tools/catch_bench.py random                               # (c) the random policy's exact expected return (no GPU)
    python tools/catch_bench.py learning --seeds 1 2 3 [--train-steps N ...]   # (c) examples/train_catch.py per seed, curves collected
    python tools/catch_bench.py bench --parent-tree DIR                        # (b) bench.py beside a built checkout of the parent commit

`move`: 512 envs, the C4 net (MuZeroAtariNet 8 x 96 x 96, 8 blocks, 128 planes, supports 61) with Catch's 3 actions, 50 simulations.
Device Catch (float32 and compact records) and Synthetic-Atari are timed with HIP events on the planner's stream (Planner.profile_*);
the host-stepped path over 512 host CatchEnv objects is wall time (it synchronises every move).  `trace` runs `move --trace-child` under
rocprofv3 --kernel-trace --stats and reads the two kernels' rows from the statistics."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
OUT_DIR = os.path.join(REPO, 'profiles', 'catch')
B, SIMS = 512, 50
NET = ('c4_catch', 'atari', (8, 96, 96), 3, 8, 128, 61, 61, 41)  # bench.py's C4 net with 3 actions


def _planner(net):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=2000, num_simulations=SIMS, discount=0.997, root_dirichlet_alpha=0.25), 0)
    p.load_state_dict(net.state_dict())
    return p


def _timed(p, steps, warmup):
    p.selfplay_step(1.0, warmup)
    p.synchronize()
    p.profile_begin()
    t0 = time.perf_counter()
    p.selfplay_step(1.0, steps)
    p.synchronize()
    wall = time.perf_counter() - t0
    prof = p.profile_end()
    return dict(ms_per_move_hip_events=prof['elapsed_ms'] / steps, ms_per_move_wall=1e3 * wall / steps,
                search_kernel_ms_per_launch=prof['search_kernel_ms'] / max(1, prof['search_kernel_launches']), steps=steps, warmup=warmup)


def move(args):
    import numpy as np
    from helpers import build_conv
    from muzero_amd import build as mz_build
    from muzero_amd import games
    from muzero_amd import planner as pl

    net = build_conv(NET)
    legs = {}
    for rec in ('f32', 'frames_u8'):
        p = _planner(net)
        p.selfplay_reset_catch(12, 12, record_format=rec)
        legs[f'device_catch_{rec}'] = dict(_timed(p, args.steps, args.warmup), record_info=p.record_info(), counters={k: int(v) for k, v in p.selfplay_counters().items()})
        p.close()
    if args.trace_child:
        return None
    p = _planner(net)
    p.selfplay_reset(pl.ENV_SYNTHETIC)
    legs['synthetic_atari'] = _timed(p, args.steps, args.warmup)
    p.close()
    for rec in ('f32', 'frames_u8'):
        p = _planner(net)
        p.selfplay_reset_external(stack_history=4, is_obs_image=True, frame_shape=(1, 96, 96), frame_u8=True, max_episode_steps=11, record_format=rec)
        envs = [games.CatchEnv(seed=e, first_row=e % 11) for e in range(B)]
        frames = np.stack([e.reset() for e in envs])
        ones, rew, done = np.ones((B, 3), np.uint8), np.zeros(B, np.float32), np.zeros(B, np.uint8)
        t_env = 0.0
        for m in range(args.warmup + args.steps):
            if m == args.warmup:
                p.synchronize()
                t0, t_env = time.perf_counter(), 0.0
            act = p.external_act(frames, ones, 1, 1, 1.0)
            t1 = time.perf_counter()
            for i, e in enumerate(envs):
                f, rew[i], d, _ = e.step(int(act[i]))
                done[i] = 1 if d else 0
                frames[i] = e.reset() if d else f
            t_env += time.perf_counter() - t1
            p.external_commit(rew, done)
        p.synchronize()
        wall = time.perf_counter() - t0
        legs[f'host_stepped_catch_{rec}'] = dict(ms_per_move_wall=1e3 * wall / args.steps, of_which_host_env_step_ms=1e3 * t_env / args.steps, steps=args.steps,
                                                 warmup=args.warmup)
        p.close()
    return dict(what=f'one self-play move, {B} envs x {SIMS} simulations, MuZeroAtariNet 8x96x96 / 8 blocks / 128 planes / supports 61 / 3 actions',
                legs=legs, _source_fingerprint=mz_build.source_fingerprint())


def trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 't', '--', sys.executable, os.path.abspath(__file__), 'move',
               '--trace-child', '--steps', str(args.steps), '--warmup', str(args.warmup)]
        subprocess.run(cmd, check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=500)
        stats = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        rows = list(csv.DictReader(open(stats[0])))
    moves = 2 * (args.steps + args.warmup)  # both record formats
    out, total = {}, 0.0
    for r in rows:
        name, ns, calls = r['Name'], float(r['TotalDurationNs']), int(r['Calls'])
        total += ns
        for k in ('k_game_step<Catch>', 'k_game_render<Catch>', 'k_game_reset<Catch>', 'k_ext_ingest', 'k_ext_commit', 'k_ext_record'):
            if all(part in name for part in k.rstrip('>').split('<')):  # (a template instance is named with its argument: both must match)
                d = out.setdefault(k, dict(calls=0, total_us=0.0))
                d['calls'] += calls
                d['total_us'] += ns / 1e3
    for d in out.values():
        d['us_per_call'] = d['total_us'] / d['calls']
    return dict(what=f'rocprofv3 --kernel-trace --stats over {moves} device Catch moves at C4 shape ({B} envs): the env kernels\' own time',
                kernels=out, all_kernels_ms_per_move=total / 1e6 / moves, moves=moves)


def random_policy(args):
    from muzero_amd.games import catch_random_policy_return

    return dict(what='expected return of the uniformly random policy on CatchEnv, exact (dynamic programming over paddle column x steps left, averaged over ball columns)',
                rows=12, cols=12, random_policy_return=catch_random_policy_return(12, 12))


def learning(args):
    from muzero_amd.games import catch_random_policy_return

    runs = []
    for seed in args.seeds:
        with tempfile.NamedTemporaryFile(suffix='.json') as f:
            cmd = [sys.executable, os.path.join(REPO, 'examples', 'train_catch.py'), '--seed', str(seed), '--train-steps', str(args.train_steps), '--envs',
                   str(args.envs), '--eval-every', str(args.eval_every), '--out', f.name] + args.extra
            t0 = time.time()
            subprocess.run(cmd, check=True, timeout=args.timeout)
            doc = json.load(open(f.name))
        runs.append(dict(seed=seed, seconds=round(time.time() - t0, 1), evals=doc['evals'], summary=doc['summary'], args={k: v for k, v in doc['args'].items() if k != 'out'}))
    rnd = catch_random_policy_return(12, 12)
    return dict(what='examples/train_catch.py per seed: greedy evaluation curves (mean return over lock-step host CatchEnv episodes, every ball column equally often)',
                random_policy_return=rnd, criterion='final eval mean return exceeds random_policy_return by more than 3 standard errors of the evaluation mean, on every seed',
                learned_on_every_seed=all(r['summary']['learned'] for r in runs), runs=runs)


def bench(args):
    """bench.py --gpus 1 in this tree and the parent's, alternating, two runs each (tools/split_atari_learner_bench.py's bench_vs_parent), then the
    parent's own run-to-run spread beside the difference."""
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import split_atari_learner_bench as sab

    out = os.path.dirname(args.out) if args.out else OUT_DIR
    sab.bench_vs_parent(os.path.abspath(args.parent_tree), out, 2)
    path = os.path.join(out, 'bench_vs_parent.json')
    doc = json.load(open(path))
    os.remove(path)
    new, par = [doc[f'new_{i}']['value'] for i in (1, 2)], [doc[f'parent_{i}']['value'] for i in (1, 2)]
    doc['headline'] = dict(metric=doc['new_1']['metric'], new=new, parent=par, parent_run_to_run_spread=abs(par[0] - par[1]),
                           new_mean_minus_parent_mean=sum(new) / 2 - sum(par) / 2)
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('move', 'trace', 'random', 'learning', 'bench'))
    ap.add_argument('--parent-tree', default='')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--trace-child', action='store_true')
    ap.add_argument('--seeds', type=int, nargs='+', default=[1, 2, 3])
    ap.add_argument('--train-steps', type=int, default=2000)
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--eval-every', type=int, default=500)
    ap.add_argument('--timeout', type=int, default=900)
    ap.add_argument('--out', default='')
    ap.add_argument('extra', nargs='*', help='after --: passed on to examples/train_catch.py')
    args = ap.parse_args()
    doc = dict(move=move, trace=trace, random=random_policy, learning=learning, bench=bench)[args.mode](args)
    if doc is None:
        return
    out = args.out or os.path.join(OUT_DIR, {'move': 'move_time.json', 'trace': 'env_kernels.json', 'random': 'random_policy.json', 'learning': 'learning.json', 'bench': 'bench_vs_parent.json'}[args.mode])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(doc, open(out, 'w'), indent=1)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
