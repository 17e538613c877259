"""What the compact record ring costs and saves: a C4-shaped host-stepped run -- 512 envs, 8 x 96 x 96 observations
(StackFrameAndAction(4) of uint8 [1, 96, 96] frames replayed from memory), make_atari_config's acc_seq_length / unroll_steps / td_steps, a
frames_u8 replay, a small Atari net and one simulation per move -- on float32 records and on compact records, and, given a checkout of
the parent commit with its libraries built, on the parent's float32 records.

    python tools/record_ring_bench.py [--parent-tree PATH] [--out-dir profiles/record_ring] [--quick] [--skip flush,ingest,memory]

One child process per (tree, record format, run); --runs runs each (default 2), the builds interleaved.  A child that fails for any
reason -- a non-zero exit status, a signal, its time limit -- ends the whole run after what was collected so far has been written: nothing
more is started on the GPU.  The one expected refusal, a reset the memory leg asks for that does not fit, is caught inside the child and
reported as a result.
  flush   HIP events on the planner's stream around mz_selfplay_external_commit (mz_profile_begin / _end) after a synchronise, for the
          move on which every env flushes acc_seq_length items: the reward / done copies, k_ext_commit, one host round trip, k_epi_scan,
          k_epi_states, k_epilogue, k_epi_publish.  Bytes: computed from the shapes, not measured -- what k_epi_states asks for (every frame
          record up to S times) and what it writes for the states, by format.
  ingest  k_ext_ingest per move from a rocprofv3 kernel trace of 24 moves.
  memory  mz_selfplay_record_info at this shape, and the largest env count of --memory-envs that mz_selfplay_reset_external accepts
          beside a 10^6-item frames_u8 replay (allocated for real), by record format."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBS, A, S, FRAME = (8, 96, 96), 18, 4, (1, 96, 96)


def _planner(args, B, cap):
    import numpy as np

    tree = os.path.abspath(args.tree) if args.tree else REPO
    sys.path[:0] = [tree, os.path.join(tree, 'tests')]
    from helpers import seeded_state_dict
    from muzero_amd import network
    from muzero_amd import planner as pl
    from muzero_amd.config import make_atari_config
    from muzero_amd.replay import PrioritizedReplay

    c = make_atari_config(use_tensorboard=False)
    cfg = types.SimpleNamespace(is_board_game=False, acc_seq_length=c.acc_seq_length, unroll_steps=c.unroll_steps, td_steps=c.td_steps, discount=0.997)
    net = network.MuZeroAtariNet(OBS, A, 1, 16, 61, 61)
    net.load_state_dict(seeded_state_dict(net, 5))
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=2, num_simulations=1, discount=0.997), 0)
    p.load_state_dict(net.state_dict())
    rp = PrioritizedReplay(cap if cap else B * cfg.acc_seq_length, 0.0, 0.0, np.random.RandomState(0), device='cuda', state_format='frames_u8',
                           frame_spec=(S,) + FRAME + (A,))
    p.attach_replay(rp, cfg, obs_shape=OBS)
    kw = dict(record_format=args.fmt) if args.fmt != 'f32' else {}  # (the parent's tree has no such keyword)
    p.selfplay_reset_external(stack_history=S, is_obs_image=True, frame_shape=FRAME, frame_u8=True, max_episode_steps=0, **kw)
    return p, rp, cfg


def child_run(args):
    import numpy as np

    B = 64 if args.quick else 512
    p, rp, cfg = _planner(args, B, 0)
    moves = 24 if args.child == 'ingest' else cfg.acc_seq_length + cfg.unroll_steps + cfg.td_steps + 2
    frames = np.random.RandomState(3).randint(0, 256, size=(8, B) + FRAME).astype(np.uint8)
    mask, per_move, items, act_ms = np.ones((B, A), np.uint8), [], [], []
    for m in range(moves):
        p.synchronize()
        p.profile_begin()
        p.external_act(frames[m % 8], mask, 1, 1, 1.0)
        act_ms.append(p.profile_end()['elapsed_ms'])
        before = rp.num_added
        p.synchronize()
        p.profile_begin()
        p.external_commit(np.ones(B, np.float32), np.zeros(B, np.uint8))
        per_move.append(p.profile_end()['elapsed_ms'])
        items.append(rp.num_added - before)
    row = int(np.prod(rp._ring['state'].shape[1:]))
    n = max(items)
    src = n * (S * int(np.prod(FRAME)) + 4 * S) if args.fmt == 'frames_u8' else n * int(np.prod(OBS)) * 4  # (from the shapes, not measured)
    quiet = sorted(t for t, k in zip(per_move, items) if k == 0)
    out = dict(fmt=args.fmt, envs=B, moves=moves, flush_items=n, flush_ms=per_move[items.index(n)] if n else None,
               state_bytes_requested_estimate=src, state_bytes_written_estimate=n * row, quiet_commit_ms_median=quiet[len(quiet) // 2], act_ms_median=sorted(act_ms[2:])[len(act_ms[2:]) // 2])
    if hasattr(p, 'record_info'):
        out['record_info'] = p.record_info()
    print(json.dumps(out))
    p.detach_replay()
    p.close()


def child_memory(args):
    try:
        p, rp, _ = _planner(args, args.envs, 10 ** 6)
    except Exception as e:  # the expected end of this leg: a planner, replay or record ring that does not fit is refused with an error
        if type(e).__name__ not in ('PlannerError', 'MemoryError', 'OutOfMemoryError'):
            raise
        print(json.dumps(dict(fmt=args.fmt, envs=args.envs, refused=f'{type(e).__name__}: {e}'[-200:])))
        return
    print(json.dumps(dict(fmt=args.fmt, envs=args.envs, record_info=p.record_info())))
    p.detach_replay()
    p.close()


def _child(args, child, fmt, tree='', extra=(), prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), '--child', child, '--fmt', fmt] + (['--quick'] if args.quick else []) + \
        (['--tree', os.path.abspath(tree)] if tree else []) + list(extra)
    r = subprocess.run(cmd, timeout=900, capture_output=True, text=True)  # (TimeoutExpired propagates: a hang ends the run)
    if r.returncode:
        raise RuntimeError(f'{child} child ({fmt}{", " + tree if tree else ""}) ended with status {r.returncode}: {r.stderr[-300:]}')
    return r


def ingest_ns(args, fmt, tree):
    with tempfile.TemporaryDirectory() as d:
        r = _child(args, 'ingest', fmt, tree, prefix=['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'g', '--'])
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                if 'k_ext_ingest' in row.get('Name', ''):
                    return dict(kernel=row['Name'][:48], calls=int(row['Calls']), mean_ns=float(row['AverageNs']), min_ns=float(row['MinNs']), max_ns=float(row['MaxNs']))
    return dict(error='k_ext_ingest not found in the kernel trace (the trace tool\'s output layout differs between ROCm releases)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-tree', default='', help='a checkout of the parent commit with its libraries built')
    ap.add_argument('--out-dir', default=os.path.join(REPO, 'profiles', 'record_ring'))
    ap.add_argument('--quick', action='store_true', help='64 envs: a check of the script, not a measurement')
    ap.add_argument('--skip', default='', help='comma list of legs to skip: flush, ingest, memory')
    ap.add_argument('--record-format', default='f32,frames_u8', help='comma list of record formats to run on this tree')
    ap.add_argument('--runs', type=int, default=2, help='runs per build in the flush and ingest legs')
    ap.add_argument('--memory-envs', default='1024,2048,3072,4096,8192,16384')
    ap.add_argument('--child', default='')
    ap.add_argument('--fmt', default='f32')
    ap.add_argument('--tree', default='')
    ap.add_argument('--envs', type=int, default=512)
    a = ap.parse_args()
    if a.child in ('flush', 'ingest'):
        return child_run(a)
    if a.child == 'memory':
        return child_memory(a)
    os.makedirs(a.out_dir, exist_ok=True)
    skip, fmts = set(a.skip.split(',')), [f for f in a.record_format.split(',') if f]
    builds = ([('parent_f32', 'f32', a.parent_tree)] if a.parent_tree else []) + [('this_' + f, f, '') for f in fmts]

    def dump(name, doc):
        with open(os.path.join(a.out_dir, name), 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')
        print(json.dumps(doc, indent=1), flush=True)

    if 'flush' not in skip:
        doc = dict(what='C4-shaped flush: mz_selfplay_external_commit of the move on which every env emits acc_seq_length items (HIP events)', quick=a.quick, runs={})
        try:
            for rep in range(a.runs):  # interleaved: every build once, then every build again
                for name, f, tree in builds:
                    doc['runs'].setdefault(name, []).append(json.loads(_child(a, 'flush', f, tree).stdout.strip().splitlines()[-1]))
        finally:  # (a failed child ends the run: what was collected is written first)
            dump('flush.json', doc)
    if 'ingest' not in skip:
        doc = dict(what='k_ext_ingest per move at the same shape (rocprofv3 kernel trace, 24 moves)', quick=a.quick, runs={})
        try:
            for rep in range(a.runs):
                for name, f, tree in builds:
                    doc['runs'].setdefault(name, []).append(ingest_ns(a, f, tree))
        finally:
            dump('ingest.json', doc)
    if 'memory' not in skip:
        doc = dict(what='largest env count mz_selfplay_reset_external accepts beside a 10^6-item frames_u8 replay (acc_seq_length 200), of ' + a.memory_envs, rows={})
        try:
            for f in fmts:
                rows = doc['rows'].setdefault(f, dict(largest_accepted=None, tries=[]))
                for envs in (int(v) for v in a.memory_envs.split(',')):
                    row = json.loads(_child(a, 'memory', f, extra=['--envs', str(envs)]).stdout.strip().splitlines()[-1])
                    rows['tries'].append(row)
                    if 'refused' in row:
                        break
                    rows['largest_accepted'] = envs
        finally:
            dump('memory.json', doc)


if __name__ == '__main__':
    main()
