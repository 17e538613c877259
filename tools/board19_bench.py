#!/usr/bin/env python3
"""C5-19: C5's self-play move on a 19 x 19 Gomoku board -- MuZeroBoardGameNet((9, 19, 19), 362 actions, 8 blocks, 128 planes), seeded
random weights, 256 envs x 200 simulations, the device Gomoku env with root noise (alpha 0.03, eps 0.25), the board temperature schedule.
Reports ms per move, simulations per second and the move's share of the fp32 MFMA peak (bench.py's conv_flops at 19 x 19: 3.815 GFLOP
per simulation, C5 2.307), for the whole-image 19 x 19 conv build (MZ_CONV_SPEC=1) and the generic path (MZ_CONV_SPEC=0, nine ragged
8 x 8 tiles per image).  MZ_CONV_SPEC is read once per process, so every leg is a fresh child process; legs alternate (spec1, spec0,
spec1, ...).  Host-inclusive wall time over `moves` moves after `warm` untimed ones.  For the per-kernel split run one leg under
`rocprofv3 --kernel-trace --stats -- python tools/board19_bench.py --child --spec 1 --moves 2 --warm 1`.

    python tools/board19_bench.py [--legs 4] [--moves 4] [--warm 1] [--out results.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

C5_19 = ('c5_19', 'board', (9, 19, 19), 362, 8, 128, 1, 1, 42)  # bench.py's C5 case, 19 x 19
B, S = 256, 200


def child(spec, moves, warm):
    import torch
    from bench import PEAK_FP32_MFMA_TFLOPS, conv_flops
    from helpers import build_conv
    from muzero_amd import build as mz_build
    from muzero_amd import planner as pl

    assert os.environ.get('MZ_CONV_SPEC', '1') == spec
    net = build_conv(C5_19)
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=1000, num_simulations=S, discount=1.0, is_board_game=True,
                                     known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.03, root_exploration_eps=0.25), 0)
    p.load_state_dict(net.state_dict())
    p.selfplay_reset(pl.ENV_GOMOKU)
    p.selfplay_step(-1.0, warm)
    p.synchronize()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.selfplay_step(-1.0, moves)
    p.synchronize()
    dt = (time.perf_counter() - t0) / moves
    sim_flop, root_flop = conv_flops(C5_19)
    flop = B * (S * sim_flop + root_flop)
    res = dict(workload='c5_19', spec=int(spec), envs=B, sims=S, moves=moves, warm=warm, ms_per_move=dt * 1e3, sims_per_s=B * S / dt,
               gflop_per_sim=sim_flop / 1e9, tflops=flop / dt / 1e12, peak=PEAK_FP32_MFMA_TFLOPS, frac=flop / dt / 1e12 / PEAK_FP32_MFMA_TFLOPS,
               counters=p.selfplay_counters(), _source_fingerprint=mz_build.source_fingerprint())
    p.close()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--spec', default='1')
    ap.add_argument('--legs', type=int, default=4)
    ap.add_argument('--moves', type=int, default=4)
    ap.add_argument('--warm', type=int, default=1)
    ap.add_argument('--out', default='')
    a = ap.parse_args()
    if a.child:
        return child(a.spec, a.moves, a.warm)
    legs = []
    for i in range(a.legs):
        spec = '1' if i % 2 == 0 else '0'
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--spec', spec, '--moves', str(a.moves), '--warm', str(a.warm)],
                           env=dict(os.environ, MZ_CONV_SPEC=spec), capture_output=True, text=True, timeout=1800)
        if r.returncode != 0:
            sys.exit(f'leg {i} (MZ_CONV_SPEC={spec}) exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
        legs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(legs[-1]), flush=True)
    summary = dict(legs=legs, _source_fingerprint=legs[0]['_source_fingerprint'])
    for spec in (1, 0):
        ms = sorted(leg['ms_per_move'] for leg in legs if leg['spec'] == spec)
        if ms:
            best = [leg for leg in legs if leg['spec'] == spec and leg['ms_per_move'] == ms[0]][0]
            summary[f'spec{spec}'] = dict(ms_per_move_min=ms[0], ms_per_move_max=ms[-1], sims_per_s=best['sims_per_s'], frac=best['frac'],
                                          tflops=best['tflops'])
    if 'spec1' in summary and 'spec0' in summary:
        summary['speedup_spec1_over_spec0'] = summary['spec0']['ms_per_move_min'] / summary['spec1']['ms_per_move_min']
    print(json.dumps({k: v for k, v in summary.items() if k != 'legs'}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(summary, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
