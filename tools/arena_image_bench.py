#!/usr/bin/env python3
"""Measurements of the image arena (mz_arena_reset_catch, mz_arena_reset_external); each mode writes one JSON file under
profiles/arena_image/ (or --out).

    python tools/arena_image_bench.py ply                        # a ply at C4 shape, three ways, same process
    python tools/arena_image_bench.py trace                      # the new kernels' own time beside the search, from a kernel trace
    python tools/arena_image_bench.py bench --parent-tree DIR    # bench.py beside a built checkout of the parent commit

`ply`: 512 games, the C4 net (MuZeroAtariNet 8 x 96 x 96, 8 blocks, 128 planes, supports 61) with Catch's 3 actions, 50 simulations, 12 x 12
Catch on 96 x 96 frames; a whole match is 11 plies.  (a) the device Catch arena, HIP events on the planner's stream (Planner.profile_*) over the
whole match, `--runs` matches (their spread is the yardstick's noise); (b) the host-stepped arena fed by 512 host CatchEnv objects, wall time
(it synchronises every ply); (c) the evaluation loop of examples/train_catch.py at the same size (512 host make_catch_env objects, host
stacking, float32 observations uploaded into Planner.search), wall time.  For reference, in the same process: a device Catch self-play move
(tools/catch_bench.py's leg).  `trace` runs `ply --trace-child` (leg (a) only) under rocprofv3 --kernel-trace --stats."""
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
OUT_DIR = os.path.join(REPO, 'profiles', 'arena_image')
B, SIMS, ROWS, COLS, S = 512, 50, 12, 12, 4
PLIES = ROWS - 1
NET = ('c4_catch', 'atari', (8, 96, 96), 3, 8, 128, 61, 61, 41)  # bench.py's C4 net with 3 actions


def _planner(net):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=2000, num_simulations=SIMS, discount=0.997, root_dirichlet_alpha=0.25), 0)
    p.load_state_dict(net.state_dict())
    return p


def _summary(res):
    return dict(mean_return=float(res['ret'].mean()), finished=int(res['draws']), finished_plies=int(res['finished_plies']), live=int(res['live']))


def _device_match(p):
    p.arena_reset_catch(ROWS, COLS)
    p.synchronize()
    p.profile_begin()
    t0 = time.perf_counter()
    p.arena_step(PLIES)
    p.synchronize()
    wall = time.perf_counter() - t0
    prof = p.profile_end()
    return dict(ms_per_ply_hip_events=prof['elapsed_ms'] / PLIES, ms_per_ply_wall=1e3 * wall / PLIES,
                search_kernel_ms_per_launch=prof['search_kernel_ms'] / max(1, prof['search_kernel_launches']), plies=PLIES, result=_summary(p.arena_result()))


def ply(args):
    import numpy as np
    from helpers import build_conv
    from muzero_amd import build as mz_build
    from muzero_amd import games

    net = build_conv(NET)
    legs = {}
    p = _planner(net)
    _device_match(p)  # warm-up match
    runs = [_device_match(p) for _ in range(args.runs)]
    p.close()
    ms = [r['ms_per_ply_hip_events'] for r in runs]
    legs['a_device_catch_arena'] = dict(runs=runs, ms_per_ply_hip_events=ms, spread_of_runs_ms=max(ms) - min(ms))
    if args.trace_child:
        return None
    # (b) the host-stepped arena over host CatchEnv objects: uint8 frames up, the device stacks
    p = _planner(net)
    p.arena_reset_external(stack_history=S, is_obs_image=True, frame_shape=(1, 96, 96), frame_u8=True)
    envs = [games.CatchEnv(ROWS, COLS, ball_cols=[e % COLS]) for e in range(B)]
    frames = np.stack([e.reset() for e in envs])
    ones, rew, done = np.ones((B, 3), np.uint8), np.zeros(B, np.float32), np.zeros(B, np.uint8)
    p.synchronize()
    t0, t_env = time.perf_counter(), 0.0
    for _ in range(PLIES):
        act, live = p.arena_external_act(frames, ones, 1, 1)
        t1 = time.perf_counter()
        for i in np.flatnonzero(live):
            frames[i], rew[i], d, _ = envs[i].step(int(act[i]))
            done[i] = 1 if d else 0
        t_env += time.perf_counter() - t1
        p.arena_external_commit(rew, done)
    p.synchronize()
    wall = time.perf_counter() - t0
    legs['b_host_stepped_arena'] = dict(ms_per_ply_wall=1e3 * wall / PLIES, of_which_host_env_step_ms=1e3 * t_env / PLIES, plies=PLIES,
                                        result=_summary(p.arena_result()))
    p.close()
    # (c) examples/train_catch.py's evaluate(): host envs, host stacking, float32 observations into Planner.search
    p = _planner(net)
    envs = [games.make_catch_env(ROWS, COLS, 8, 8, stack_history=S) for _ in range(B)]
    obs = np.stack([e.reset(ball_col=i % COLS) for i, e in enumerate(envs)])
    mask = np.ones((B, 3), bool)
    rets = np.zeros(B)
    p.synchronize()
    t0 = time.perf_counter()
    for _ in range(PLIES):
        act = p.search(obs, mask, 1, 1, 0.0, deterministic=True)['action']
        nxt = []
        for i, e in enumerate(envs):
            o, r, _, _ = e.step(int(act[i]))
            rets[i] += r
            nxt.append(o)
        obs = np.stack(nxt)
    wall = time.perf_counter() - t0
    legs['c_example_host_loop'] = dict(ms_per_ply_wall=1e3 * wall / PLIES, plies=PLIES, observation_bytes_uploaded_per_ply=int(obs.nbytes),
                                       result=dict(mean_return=float(rets.mean())))
    p.close()
    # the yardstick in the same process: a device Catch self-play move (float32 records), tools/catch_bench.py's leg
    p = _planner(net)
    p.selfplay_reset_catch(ROWS, COLS)
    p.selfplay_step(1.0, 2)
    p.synchronize()
    p.profile_begin()
    p.selfplay_step(1.0, 8)
    p.synchronize()
    prof = p.profile_end()
    legs['selfplay_move_same_process'] = dict(ms_per_move_hip_events=prof['elapsed_ms'] / 8, steps=8, warmup=2)
    p.close()
    recorded = None
    path = os.path.join(REPO, 'profiles', 'catch', 'move_time.json')
    if os.path.exists(path):
        recorded = json.load(open(path))['legs']['device_catch_f32']['ms_per_move_hip_events']
    a = sum(ms) / len(ms)
    return dict(what=f'one arena ply, {B} games x {SIMS} simulations, MuZeroAtariNet 8x96x96 / 8 blocks / 128 planes / supports 61 / 3 actions, {ROWS} x {COLS} Catch',
                legs=legs,
                arena_ply_minus_selfplay_move_ms=dict(same_process=a - legs['selfplay_move_same_process']['ms_per_move_hip_events'],
                                                      recorded_profiles_catch=None if recorded is None else a - recorded,
                                                      spread_of_two_arena_runs_ms=legs['a_device_catch_arena']['spread_of_runs_ms']),
                _source_fingerprint=mz_build.source_fingerprint())


KERNELS = ('k_imgarena_ingest', 'k_game_arena_step<Catch>', 'k_imgarena_record', 'k_imgarena_commit', 'k_imgarena_reset', 'k_game_reset<Catch>', 'k_arena_pre',
           'k_game_render<Catch>')


def trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 't', '--', sys.executable, os.path.abspath(__file__), 'ply',
               '--trace-child', '--runs', str(args.runs)]
        subprocess.run(cmd, check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=500)
        stats = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        rows = list(csv.DictReader(open(stats[0])))
    plies = PLIES * (args.runs + 1)  # (the warm-up match too)
    out, total = {}, 0.0
    for r in rows:
        name, ns, calls = r['Name'], float(r['TotalDurationNs']), int(r['Calls'])
        total += ns
        for k in KERNELS:
            if all(part in name for part in k.rstrip('>').split('<')):  # (a template instance is named with its argument: both must match)
                d = out.setdefault(k, dict(calls=0, total_us=0.0))
                d['calls'] += calls
                d['total_us'] += ns / 1e3
    for d in out.values():
        d['us_per_call'] = d['total_us'] / d['calls']
    per_ply = sum(d['total_us'] for k, d in out.items() if k not in ('k_imgarena_reset', 'k_game_reset<Catch>')) / plies
    return dict(what=f'rocprofv3 --kernel-trace --stats over {plies} device Catch arena plies at C4 shape ({B} games): the arena kernels\' own time beside the search',
                kernels=out, arena_kernels_us_per_ply=per_ply, all_kernels_ms_per_ply=total / 1e6 / plies, plies=plies)


def bench(args):
    """bench.py --gpus 1 in this tree and the parent's, alternating, two runs each, then --dump-outputs of C2, C3, C5 and lunar compared byte
    for byte (tools/split_atari_learner_bench.py's bench_vs_parent); the parent's own run-to-run spread beside the difference."""
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
    ap.add_argument('mode', choices=('ply', 'trace', 'bench'))
    ap.add_argument('--parent-tree', default='')
    ap.add_argument('--runs', type=int, default=2)
    ap.add_argument('--trace-child', action='store_true')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    doc = dict(ply=ply, trace=trace, bench=bench)[args.mode](args)
    if doc is None:
        return
    out = args.out or os.path.join(OUT_DIR, dict(ply='ply_time.json', trace='arena_kernels.json', bench='bench_vs_parent.json')[args.mode])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(doc, open(out, 'w'), indent=1)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
