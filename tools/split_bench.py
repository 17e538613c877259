#!/usr/bin/env python3
"""Split-bf16 conv inference against the float32 path: C5 (Gomoku 15 x 15) and C5-19 (19 x 19), MuZeroBoardGameNet with 128 planes x 8
blocks, seeded random weights, 256 envs x 200 simulations, the device Gomoku env with root noise (alpha 0.03, eps 0.25), the board
temperature schedule.  Per (workload, conv_precision): ms per self-play move (host-inclusive wall time over `moves` moves after `warm`
untimed ones) and, with --layers, the average time of one conv launch from a `rocprofv3 --kernel-trace --stats` run of one move (no
counters in that trace).  Every leg is a fresh child process; legs alternate between the modes.

    python tools/split_bench.py [--legs 2] [--moves 2] [--warm 1] [--layers] [--out profiles/split_bf16]

--fp32-only (with --out FILE.json) times the float32 legs alone: run from a checkout of the parent commit it gives the parent's numbers on
the same box (the parent has no conv_precision field; the flag keeps it out of the config)."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

CASES = {
    'c5': ('c5', 'board', (9, 15, 15), 226, 8, 128, 1, 1, 42),
    'c5_19': ('c5_19', 'board', (9, 19, 19), 362, 8, 128, 1, 1, 42),
}
B, S = 256, 200


def child(workload, mode, moves, warm):
    import torch
    from helpers import build_conv
    from muzero_amd import build as mz_build
    from muzero_amd import planner as pl

    net = build_conv(CASES[workload])
    kw = dict(num_envs=B, seed=1000, num_simulations=S, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.03,
              root_exploration_eps=0.25)
    if mode != 'f32-parent':
        kw['conv_precision'] = mode
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, **kw), 0)
    p.load_state_dict(net.state_dict())
    p.selfplay_reset(pl.ENV_GOMOKU)
    if warm:
        p.selfplay_step(-1.0, warm)
    p.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.selfplay_step(-1.0, moves)
    p.synchronize()
    dt = (time.perf_counter() - t0) / moves
    res = dict(workload=workload, mode=mode, envs=B, sims=S, moves=moves, warm=warm, ms_per_move=dt * 1e3, sims_per_s=B * S / dt,
               describe=p.describe(), counters=p.selfplay_counters(), _source_fingerprint=mz_build.source_fingerprint())
    p.close()
    print(json.dumps(res), flush=True)


def run_child(workload, mode, moves, warm, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), '--child', '--workload', workload, '--mode', mode, '--moves', str(moves), '--warm', str(warm)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f'{workload} / {mode} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


def conv_layer_times(workload, mode, keep_csv=''):
    """One move under rocprofv3 --kernel-trace --stats: [(kernel, calls, average us)] of the conv kernels, most time first."""
    d = tempfile.mkdtemp(prefix='split_trace_')
    try:
        run_child(workload, mode, 1, 0, prefix=['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 't', '--'])
        stats = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if not stats:
            sys.exit(f'no kernel_stats.csv under {d}')
        if keep_csv:
            shutil.copyfile(stats[0], keep_csv)
        rows = list(csv.DictReader(open(stats[0])))
        total = sum(float(r['TotalDurationNs']) for r in rows)
        conv = [dict(kernel=r['Name'], calls=int(r['Calls']), avg_us=float(r['AverageNs']) / 1e3, share=float(r['TotalDurationNs']) / total)
                for r in rows if 'k_conv3x3' in r['Name']]
        return sorted(conv, key=lambda c: -c['share'])
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--workload', default='c5')
    ap.add_argument('--mode', default='f32')
    ap.add_argument('--legs', type=int, default=2, help='timed legs per (workload, mode)')
    ap.add_argument('--moves', type=int, default=2)
    ap.add_argument('--warm', type=int, default=1)
    ap.add_argument('--layers', action='store_true', help='per-conv-launch times from a rocprofv3 kernel trace of one move per (workload, mode)')
    ap.add_argument('--fp32-only', action='store_true')
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.child:
        return child(a.workload, a.mode, a.moves, a.warm)
    modes = ['f32-parent'] if a.fp32_only else ['f32', 'bf16x3']
    summary = {}
    for w in CASES:
        legs = []
        for i in range(a.legs):
            for mode in modes:
                legs.append(run_child(w, mode, a.moves, a.warm))
                print(json.dumps(legs[-1]), flush=True)
        s = dict(legs=legs)
        for mode in modes:
            ms = sorted(leg['ms_per_move'] for leg in legs if leg['mode'] == mode)
            s[mode] = dict(ms_per_move_min=ms[0], ms_per_move_max=ms[-1])
        if not a.fp32_only:
            s['speedup_bf16x3_over_f32'] = s['f32']['ms_per_move_min'] / s['bf16x3']['ms_per_move_min']
            if a.layers:
                for mode in modes:
                    keep = os.path.join(a.out, f'kernel_stats_{w}_{mode}.csv') if a.out and mode == 'bf16x3' else ''
                    if keep:
                        os.makedirs(a.out, exist_ok=True)
                    s[mode]['conv_launches'] = conv_layer_times(w, mode, keep)
        summary[w] = s
        print(json.dumps({w: {k: v for k, v in s.items() if k != 'legs'}}), flush=True)
    if a.out:
        path = a.out if a.out.endswith('.json') else os.path.join(a.out, 'split_vs_f32.json')
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        json.dump(summary, open(path, 'w'), indent=1)


if __name__ == '__main__':
    main()
