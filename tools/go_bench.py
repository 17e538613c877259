#!/usr/bin/env python3
"""Measurements of the device Go env (MZ_ENV_GO); each mode writes one JSON file under profiles/go/ (or --out).  The procedure is
tools/othello_bench.py's, whose helpers this tool uses.

    python tools/go_bench.py move     [--steps 8 --warmup 2]   # one self-play move: C5's net class on 9 x 9 and 19 x 19, Gomoku beside it, the example's net
    python tools/go_bench.py trace                             # the env kernels' own time from a kernel trace: mid-game moves and the spiral worst case
    python tools/go_bench.py learning --seeds 1 2 3 [--resign]    # examples/train_go.py per seed, arena results collected
    python tools/go_bench.py bench --parent-tree DIR           # bench.py beside a built checkout of the parent commit
    python tools/go_bench.py machine --parent-tree DIR         # the planner library's kernels against the parent's, symbol by symbol (no GPU)
    python tools/go_bench.py random                            # uniformly random play against itself on the example's board (no GPU)

`move`: 256 envs x 200 simulations, a board conv net of 128 planes x 8 blocks on (9, n, n) with n * n + 2 actions, n = 9 and 19, timed with
HIP events on the planner's stream (Planner.profile_*); a device Gomoku move of the same net class on the same board in the same process;
then the example's small net (32 planes x 2 blocks, 32 simulations, 7 x 7).  `trace` runs `move --trace-child` under rocprofv3
--kernel-trace and reads the env kernels' per-launch rows; its child also plays the two spirals of tests/go_cases.py through the debug
step, whose last plies are the longest propagations the boards allow.  The launches of a kernel come in the child's known order, so each
is attributed to its board (9 x 9, 19 x 19) and to the searched moves or the spiral.  `random` recomputes profiles/go/random_policy.json
on the host (tests/test_go_host.py holds the file to it)."""
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
sys.path.insert(0, os.path.join(REPO, 'tools'))
OUT_DIR = os.path.join(REPO, 'profiles', 'go')

import othello_bench as ob  # noqa: E402

WARMUP = 8  # moves before the timed ones of every leg: the timed moves start from positions with stones on the board


def _spirals():
    """The two spiral games through the debug step, 256 envs each playing the same game: every k_go_step launch does one position's work
    in all its workgroups, the last one the capture of the whole arm."""
    import numpy as np

    import go_cases as gc

    for name in ('spiral_9x9', 'spiral_19x19'):
        c = gc.BY_NAME[name]
        n = c['rows']
        p = ob._planner((9, n, n), n * n + 2, 8, 1, 256, 8, 54)
        p.selfplay_reset_go()
        for ply in c['plies']:
            p.debug_go_step(np.full(256, gc.action_of(c, ply[0]), np.int32))
        p.synchronize()
        p.close()


def move(args):
    from muzero_amd import build as mz_build
    from muzero_amd import planner as pl

    legs = {}
    for n in (9, 19):
        p = ob._planner((9, n, n), n * n + 2, 128, 8, 256, 200, 51)
        p.selfplay_reset_go(allow_resign=False)  # (no resignation: the warm-up moves put stones on the board before the timed ones)
        legs[f'go_{n}x{n}_c5_net'] = ob._timed(p, args.steps, max(args.warmup, WARMUP))
        p.close()
        p = ob._planner((9, n, n), n * n + 1, 128, 8, 256, 200, 52)
        p.selfplay_reset(pl.ENV_GOMOKU)
        legs[f'gomoku_{n}x{n}_c5_net'] = ob._timed(p, args.steps, max(args.warmup, WARMUP))
        p.close()
    p = ob._planner((9, 7, 7), 51, 32, 2, 256, 32, 53)
    p.selfplay_reset_go(allow_resign=False)
    legs['go_7x7_example_net'] = ob._timed(p, args.steps, max(args.warmup, WARMUP))
    p.close()
    for leg in legs.values():
        leg['search_share'] = leg['search_kernel_ms'] / leg['ms_per_move_hip_events']
    if args.trace_child:
        _spirals()
        return None
    return dict(what='one self-play move, 256 envs: board conv nets of 128 planes x 8 blocks at 200 simulations on Go 9 x 9 (83 actions) and 19 x 19 (363) and on '
                     'device Gomoku on the same boards (82 / 362 actions), and the example\'s 32 planes x 2 blocks at 32 simulations on Go 7 x 7 (51 actions); HIP '
                     'events on the planner\'s stream over `steps` moves after 8 warm-up moves, the resignation off; search_share = search kernels / whole move',
                legs=legs, _source_fingerprint=mz_build.source_fingerprint())


def trace(args):
    """Per-launch rows of the kernel trace, not the --stats summary: the child's launches of a kernel come in a known order (the legs of
    `move`, then the two spirals), so every launch is attributed to its board size and to 'moves of a game' or 'spiral'."""
    W = max(args.warmup, WARMUP)
    n = W + args.steps
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', tmp, '-o', 't', '--', sys.executable, os.path.abspath(__file__), 'move',
               '--trace-child', '--steps', str(args.steps), '--warmup', str(args.warmup)]
        subprocess.run(cmd, check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        files = glob.glob(os.path.join(tmp, '**', '*kernel_trace.csv'), recursive=True)
        rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    launches = {}
    for r in rows:
        name = r['Kernel_Name']
        for k in ('k_go_step', 'k_go_pre', 'k_env_step', 'k_env_pre'):
            if name.startswith(k) or f' {k}(' in name or f'::{k}' in name:
                launches.setdefault(k, []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    import go_cases as gc

    s9, s19 = len(gc.BY_NAME['spiral_9x9']['plies']), len(gc.BY_NAME['spiral_19x19']['plies'])
    # the child's order: Go 9 x 9, Gomoku 9 x 9, Go 19 x 19, Gomoku 19 x 19, Go 7 x 7 (n moves each), then the spirals on 9 x 9 and 19 x 19
    cuts = {'go': [('9x9', n), ('19x19', n), ('7x7', n), ('spiral_9x9', s9), ('spiral_19x19', s19)], 'env': [('9x9', n), ('19x19', n)]}
    out = {}
    for k, us in launches.items():
        plan = cuts['go' if k.startswith('k_go') else 'env']
        assert len(us) == sum(c for _, c in plan), (k, len(us), plan)
        at = 0
        for leg, c in plan:
            part = us[at:at + c]
            at += c
            if leg.startswith('spiral'):
                out[f'{k} {leg}'] = dict(launches=c, mean_us=sum(part) / c, min_us=min(part), max_us=max(part), last_ply_us=part[-1])
            else:  # the timed moves only: after the warm-up the boards hold stones
                part = part[W:]
                out[f'{k} {leg} moves {W + 1}..{n}'] = dict(launches=len(part), mean_us=sum(part) / len(part), min_us=min(part), max_us=max(part))
    return dict(what='rocprofv3 --kernel-trace, per-launch rows: the env kernels\' own time per move of 256 envs.  k_go_* are Go\'s (one workgroup per env), '
                     'k_env_* device Gomoku\'s on the same boards with the same net class, all in one traced process.  "moves a..b": the searched '
                     'self-play moves of `move`\'s legs after the warm-up moves (positions with a..b - 1 plies played, passes included).  '
                     '"spiral": the spiral game of tests/go_cases.py played by all 256 envs through the debug step; last_ply_us is the capture of the '
                     'whole arm (49 stones on 9 x 9, 199 on 19 x 19), the longest propagation the board allows',
                kernels=out)


def random_policy_stats(rows=7, cols=7, komi2=15, games=1000, seed=1):
    """Uniformly random play against itself on the host env: every ply drawn uniformly from the legal placements and the pass, never the
    resignation -- the arena's random opponent on both sides."""
    import numpy as np

    from muzero_amd.games import GoEnv

    rs = np.random.RandomState(seed)
    res, lengths, two_pass = [0, 0, 0], [], 0
    for _ in range(games):
        e = GoEnv(rows, cols, komi2=komi2, allow_resign=False)
        done = False
        while not done:
            legal = np.flatnonzero(e.actions_mask[:rows * cols + 1])
            _, _, done, _ = e.step(int(legal[rs.randint(len(legal))]))
        res[0 if e.winner == 1 else 2 if e.winner == 2 else 1] += 1
        lengths.append(e.steps)
        two_pass += e.steps < e.max_plies
    return dict(rows=rows, cols=cols, komi2=komi2, max_plies=2 * rows * cols, games=games, seed=seed,
                policy='uniform over the legal placements and the pass, never the resignation (the arena\'s random opponent)',
                first_player_win=res[0] / games, draw=res[1] / games, first_player_loss=res[2] / games, mean_length=float(np.mean(lengths)),
                min_length=int(min(lengths)), max_length=int(max(lengths)), two_pass_ends=two_pass / games)


def learning(args):
    rnd = json.load(open(os.path.join(OUT_DIR, 'random_policy.json')))
    runs = []
    n = args.arena_eval

    def score(rec):  # (wins + draws / 2) / games against the random opponent, and its standard error
        v = rec['vs_random']
        m = (v['win'] + 0.5 * v['draw']) / n
        var = (v['win'] * (1 - m) ** 2 + v['draw'] * (0.5 - m) ** 2 + v['loss'] * (0 - m) ** 2) / n
        return m, (var / n) ** 0.5

    for seed in args.seeds:
        with tempfile.NamedTemporaryFile(suffix='.json') as f:
            cmd = [sys.executable, os.path.join(REPO, 'examples', 'train_go.py'), '--seed', str(seed), '--train-steps', str(args.train_steps), '--envs',
                   str(args.envs), '--report-every', str(args.report_every), '--arena-eval', str(n), '--out', f.name] + args.extra
            t0 = time.time()
            subprocess.run(cmd, check=True, timeout=args.timeout)
            doc = json.load(open(f.name))
        log = doc['log']
        m0, se0 = score(log[0])
        first = next((rec['train_steps'] for rec in log[1:] if score(rec)[0] - m0 > 3 * (score(rec)[1] ** 2 + se0 ** 2) ** 0.5), None)
        m1, se1 = score(log[-1])
        runs.append(dict(seed=seed, seconds=round(time.time() - t0, 1), log=log, untrained_score=m0, final_score=m1, final_standard_error=se1,
                         final_exceeds_untrained_by_standard_errors=(m1 - m0) / max((se0 ** 2 + se1 ** 2) ** 0.5, 1e-12), first_report_3_se_above_untrained=first,
                         learned=bool(m1 - m0 > 3 * (se0 ** 2 + se1 ** 2) ** 0.5), args={k: v for k, v in doc['args'].items() if k != 'out'}))
        json.dump(dict(partial=True, runs=runs), open(args.out or os.path.join(OUT_DIR, 'learning.json'), 'w'), indent=1)  # (kept if a later seed is cut)
    return dict(what='examples/train_go.py per seed: win / draw / loss of the deterministic search against the uniformly random opponent (may pass, never resigns) and '
                     'against the previous checkpoint on the device arena, colours balanced, two random opening plies per pair',
                random_policy_against_itself=rnd,
                criterion='score (wins + draws / 2) / games against the random opponent exceeds the untrained net\'s by more than 3 standard errors (both combined)',
                learned_on_every_seed=all(r['learned'] for r in runs), runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('move', 'trace', 'learning', 'bench', 'machine', 'random'))
    ap.add_argument('--parent-tree', default='')
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--trace-child', action='store_true')
    ap.add_argument('--seeds', type=int, nargs='+', default=[1, 2, 3])
    ap.add_argument('--train-steps', type=int, default=1500)
    ap.add_argument('--envs', type=int, default=256)
    ap.add_argument('--report-every', type=int, default=250)
    ap.add_argument('--arena-eval', type=int, default=256)
    ap.add_argument('--timeout', type=int, default=600)
    ap.add_argument('--out', default='')
    ap.add_argument('--resign', action='store_true', help='learning: run examples/train_go.py with --resign (the resignation legal)')
    args = ap.parse_args()
    args.extra = ['--resign'] if args.resign else []
    if args.mode == 'bench' and not args.out:
        args.out = os.path.join(OUT_DIR, 'bench_vs_parent.json')
    doc = dict(move=move, trace=trace, learning=learning, bench=ob.bench, machine=ob.machine, random=lambda a: random_policy_stats())[args.mode](args)
    if doc is None:
        return
    out = args.out or os.path.join(OUT_DIR, {'move': 'move_time.json', 'trace': 'env_kernels.json', 'learning': 'learning.json', 'bench': 'bench_vs_parent.json',
                                             'machine': 'machine_code.json', 'random': 'random_policy.json'}[args.mode])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(doc, open(out, 'w'), indent=1)
    print(json.dumps(doc)[:3000])


if __name__ == '__main__':
    main()
