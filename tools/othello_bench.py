#!/usr/bin/env python3
"""Measurements of the device Othello env (MZ_ENV_OTHELLO); each mode writes one JSON file under profiles/othello/ (or --out).

    python tools/othello_bench.py move     [--steps 8 --warmup 2]   # one self-play move: C5's net class on 8 x 8, Gomoku 8 x 8 beside it, the example's net
    python tools/othello_bench.py trace                             # the env kernels' own time from a kernel trace (Othello and Gomoku)
    python tools/othello_bench.py learning --seeds 1 2 3            # examples/train_othello.py per seed, arena results collected
    python tools/othello_bench.py bench --parent-tree DIR           # bench.py beside a built checkout of the parent commit
    python tools/othello_bench.py machine --parent-tree DIR         # the planner library's kernels against the parent's, symbol by symbol (no GPU)

`move`: 256 envs x 200 simulations, a board conv net of 128 planes x 8 blocks on (9, 8, 8) with 66 actions, timed with HIP events on the
planner's stream (Planner.profile_*); a device Gomoku move of the same net class on the same board, 8 x 8 with 65 actions, in the same
process; then the example's small net (32 planes x 2 blocks, 32 simulations, 6 x 6).  `trace` runs `move --trace-child` under
rocprofv3 --kernel-trace --stats and reads the env kernels' rows from the statistics."""
import argparse
import csv
import glob
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
OUT_DIR = os.path.join(REPO, 'profiles', 'othello')
KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25)


def _planner(shape, A, planes, blocks, B, sims, seed):
    from helpers import seeded_state_dict
    from muzero_amd import planner as pl
    from muzero_amd.network import MuZeroBoardGameNet

    net = MuZeroBoardGameNet(shape, A, blocks, planes)
    net.load_state_dict(seeded_state_dict(net, seed))
    net.eval()
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=2000, num_simulations=sims, **KW), 0)
    p.load_state_dict(net.state_dict())
    return p


def _timed(p, steps, warmup):
    p.selfplay_step(-1.0, warmup)
    p.synchronize()
    p.profile_begin()
    t0 = time.perf_counter()
    p.selfplay_step(-1.0, steps)
    p.synchronize()
    wall = time.perf_counter() - t0
    prof = p.profile_end()
    return dict(ms_per_move_hip_events=prof['elapsed_ms'] / steps, ms_per_move_wall=1e3 * wall / steps, search_kernel_ms=prof['search_kernel_ms'] / steps,
                search_kernel_launches_per_move=prof['search_kernel_launches'] / steps, steps=steps, warmup=warmup, build=p.describe())


def move(args):
    from muzero_amd import build as mz_build
    from muzero_amd import planner as pl

    legs = {}
    p = _planner((9, 8, 8), 66, 128, 8, 256, 200, 51)
    p.selfplay_reset_othello()
    legs['othello_8x8_c5_net'] = _timed(p, args.steps, args.warmup)
    p.close()
    p = _planner((9, 8, 8), 65, 128, 8, 256, 200, 52)
    p.selfplay_reset(pl.ENV_GOMOKU)
    legs['gomoku_8x8_c5_net'] = _timed(p, args.steps, args.warmup)
    p.close()
    p = _planner((9, 6, 6), 38, 32, 2, 256, 32, 53)
    p.selfplay_reset_othello()
    legs['othello_6x6_example_net'] = _timed(p, args.steps, args.warmup)
    p.close()
    for leg in legs.values():
        leg['search_share'] = leg['search_kernel_ms'] / leg['ms_per_move_hip_events']
    if args.trace_child:
        return None
    return dict(what='one self-play move, 256 envs: board conv nets of 128 planes x 8 blocks at 200 simulations on Othello 8 x 8 (66 actions) and on device '
                     'Gomoku 8 x 8 (65 actions), and the example\'s 32 planes x 2 blocks at 32 simulations on Othello 6 x 6 (38 actions); HIP events on the '
                     'planner\'s stream; search_share = search kernels / whole move',
                legs=legs, _source_fingerprint=mz_build.source_fingerprint())


def trace(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', tmp, '-o', 't', '--', sys.executable, os.path.abspath(__file__), 'move',
               '--trace-child', '--steps', str(args.steps), '--warmup', str(args.warmup)]
        subprocess.run(cmd, check=True, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=500)
        stats = glob.glob(os.path.join(tmp, '**', '*kernel_stats.csv'), recursive=True)
        rows = list(csv.DictReader(open(stats[0])))
    out, total = {}, 0.0
    for r in rows:
        name, ns, calls = r['Name'], float(r['TotalDurationNs']), int(r['Calls'])
        total += ns
        for k in ('k_oth_step', 'k_oth_pre', 'k_oth_reset', 'k_env_step', 'k_env_pre', 'k_env_reset'):
            if name.startswith(k) or f' {k}(' in name or f'::{k}' in name:
                d = out.setdefault(k, dict(calls=0, total_us=0.0))
                d['calls'] += calls
                d['total_us'] += ns / 1e3
    for d in out.values():
        d['us_per_call'] = d['total_us'] / d['calls']
    moves = args.steps + args.warmup
    return dict(what=f'rocprofv3 --kernel-trace --stats over {moves} moves of each leg of `move` (256 envs): the env kernels\' own time; k_oth_* are Othello\'s '
                     '(two planners), k_env_* the Gomoku leg\'s 16-lane-group step', kernels=out, all_kernels_ms=total / 1e6, moves_per_planner=moves)


def learning(args):
    rnd = json.load(open(os.path.join(OUT_DIR, 'random_policy.json')))
    runs = []
    for seed in args.seeds:
        with tempfile.NamedTemporaryFile(suffix='.json') as f:
            cmd = [sys.executable, os.path.join(REPO, 'examples', 'train_othello.py'), '--seed', str(seed), '--train-steps', str(args.train_steps), '--envs',
                   str(args.envs), '--report-every', str(args.report_every), '--arena-eval', str(args.arena_eval), '--out', f.name] + args.extra
            t0 = time.time()
            subprocess.run(cmd, check=True, timeout=args.timeout)
            doc = json.load(open(f.name))
        log = doc['log']
        n = args.arena_eval

        def score(rec):  # (wins + draws / 2) / games against the random opponent, and its standard error
            v = rec['vs_random']
            m = (v['win'] + 0.5 * v['draw']) / n
            var = (v['win'] * (1 - m) ** 2 + v['draw'] * (0.5 - m) ** 2 + v['loss'] * (0 - m) ** 2) / n
            return m, (var / n) ** 0.5

        m0, se0 = score(log[0])
        first = next((rec['train_steps'] for rec in log[1:] if score(rec)[0] - m0 > 3 * (score(rec)[1] ** 2 + se0 ** 2) ** 0.5), None)
        m1, se1 = score(log[-1])
        runs.append(dict(seed=seed, seconds=round(time.time() - t0, 1), log=log, untrained_score=m0, final_score=m1, final_standard_error=se1,
                         final_exceeds_untrained_by_standard_errors=(m1 - m0) / max((se0 ** 2 + se1 ** 2) ** 0.5, 1e-12), first_report_3_se_above_untrained=first,
                         learned=bool(m1 - m0 > 3 * (se0 ** 2 + se1 ** 2) ** 0.5), args={k: v for k, v in doc['args'].items() if k != 'out'}))
        json.dump(dict(partial=True, runs=runs), open(args.out or os.path.join(OUT_DIR, 'learning.json'), 'w'), indent=1)  # (kept if a later seed is cut)
    return dict(what='examples/train_othello.py per seed: win / draw / loss of the deterministic search against the uniformly random opponent (passes where it must, never resigns) and '
                     'against the previous checkpoint on the device arena, colours balanced, two random opening plies per pair',
                random_policy_against_itself=rnd,
                criterion='score (wins + draws / 2) / games against the random opponent exceeds the untrained net\'s by more than 3 standard errors (both combined)',
                learned_on_every_seed=all(r['learned'] for r in runs), runs=runs)


def bench(args):
    """bench.py --gpus 1 in this tree and the parent's, alternating, two runs each (tools/split_atari_learner_bench.py's bench_vs_parent)."""
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


def _kernel_hashes(lib):
    """{function symbol: sha256 of its bytes in .text} of the gfx950 code object inside `lib`."""
    llvm = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
    with tempfile.TemporaryDirectory() as tmp:
        fat, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'gfx950.co')
        subprocess.run([os.path.join(llvm, 'llvm-objcopy'), '--dump-section', f'.hip_fatbin={fat}', lib, os.path.join(tmp, 'copy.so')], check=True)
        subprocess.run([os.path.join(llvm, 'clang-offload-bundler'), '--unbundle', '--type=o', f'--input={fat}', f'--output={co}',
                        '--targets=hipv4-amdgcn-amd-amdhsa--gfx950'], check=True)
        text = os.path.join(tmp, 'text')
        subprocess.run([os.path.join(llvm, 'llvm-objcopy'), '--dump-section', f'.text={text}', co, os.path.join(tmp, 'copy.co')], check=True)
        code = open(text, 'rb').read()
        sections = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '-S', '-W', co], check=True, capture_output=True, text=True).stdout
        base = next(int(ln.split()[ln.split().index('.text') + 2], 16) for ln in sections.splitlines() if ' .text ' in ln)
        syms = subprocess.run([os.path.join(llvm, 'llvm-readelf'), '-s', '-W', co], check=True, capture_output=True, text=True).stdout
    out = {}
    for ln in syms.splitlines():
        f = ln.split()
        if len(f) >= 8 and f[3] == 'FUNC' and f[6] != 'UND':
            addr, size = int(f[1], 16) - base, int(f[2])
            out[f[7]] = hashlib.sha256(code[addr:addr + size]).hexdigest()
    return out


def machine(args):
    new = _kernel_hashes(os.path.join(REPO, 'muzero_amd', 'lib', 'libmzplanner_hip.so'))
    par = _kernel_hashes(os.path.join(os.path.abspath(args.parent_tree), 'muzero_amd', 'lib', 'libmzplanner_hip.so'))
    demangle = lambda names: subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.split('\n')[:len(names)] if names else []  # noqa: E731
    different = sorted(k for k in par if k in new and new[k] != par[k])
    return dict(what='every function symbol of the gfx950 code object in libmzplanner_hip.so, this commit against a build of the parent commit with the same flags: '
                     'sha256 of each symbol\'s bytes in .text (llvm-objcopy --dump-section .hip_fatbin, clang-offload-bundler --unbundle, llvm-readelf -s)',
                parent_kernels=len(par), new_kernels=len(new), byte_identical=sum(1 for k in par if new.get(k) == par[k]), different=demangle(different),
                only_in_parent=demangle(sorted(k for k in par if k not in new)), only_in_new=demangle(sorted(k for k in new if k not in par)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=('move', 'trace', 'learning', 'bench', 'machine'))
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
    ap.add_argument('extra', nargs='*', help='after --: passed on to examples/train_othello.py')
    args = ap.parse_args()
    doc = dict(move=move, trace=trace, learning=learning, bench=bench, machine=machine)[args.mode](args)
    if doc is None:
        return
    out = args.out or os.path.join(OUT_DIR, {'move': 'move_time.json', 'trace': 'env_kernels.json', 'learning': 'learning.json', 'bench': 'bench_vs_parent.json',
                                             'machine': 'machine_code.json'}[args.mode])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    json.dump(doc, open(out, 'w'), indent=1)
    print(json.dumps(doc)[:3000])


if __name__ == '__main__':
    main()
