"""What the compact replay states cost and save: the device time of the epilogue launches, the learner's gather kernel and the largest
ring that fits, for this tree's float32 path, its compact path and -- given the parent commit's libraries -- the parent's float32 path.

    python tools/replay_codec_bench.py [--parent-planner-lib PATH/libmzplanner_hip.so] [--out-dir profiles/replay_codec] [--quick]

One child process per (case, build, format, run): a process loads one library.  Two runs each.
  atari   a C4-shaped host-stepped run: 512 envs, 8 x 96 x 96 observations (StackFrameAndAction(4) of uint8 [1, 96, 96] frames replayed from
          memory), make_atari_config's acc_seq_length / unroll_steps / td_steps, a small Atari net and one simulation per move (the epilogue does
          not run the net).  No episode ends: every env flushes acc_seq_length items on the same move.
  gomoku  128 host-stepped envs with whole (9, 15, 15) observations of 0 / 1 planes, Monte-Carlo targets, staggered episode ends.
Timing: HIP events on the planner's stream around mz_selfplay_external_commit (mz_profile_begin / _end) after a synchronise: the reward / done
copies, k_ext_commit, one host round trip, then the epilogue launches (k_epi_scan, k_epi_states, k_epilogue, k_epi_publish).
  gather  k_lc_gather at batch 128 over a ring of each format (this tree), from a rocprofv3 kernel trace of mzl_grad calls.
  ring    the largest capacity PrioritizedReplay.allocate accepts for 8 x 96 x 96 states in each format on this GPU (allocated for real)."""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATARI_OBS, ATARI_A, S = (8, 96, 96), 18, 4


def _setup(args):
    sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
    from muzero_amd import hip_learner as hlm
    from muzero_amd import planner as pl

    if args.planner_lib:
        pl.LIB_PATH = args.planner_lib
    if args.learner_lib:
        hlm.LIB_PATH = args.learner_lib
    return pl, hlm


def child_epilogue(args):
    import numpy as np

    pl, _ = _setup(args)
    from helpers import seeded_state_dict
    from muzero_amd import network
    from muzero_amd.config import make_atari_config
    from muzero_amd.replay import PrioritizedReplay

    fmt = None if args.fmt == 'f32' else args.fmt
    rs = np.random.RandomState(3)
    if args.child == 'atari':
        B = 64 if args.quick else 512
        c = make_atari_config(use_tensorboard=False)
        cfg = types.SimpleNamespace(is_board_game=False, acc_seq_length=c.acc_seq_length, unroll_steps=c.unroll_steps, td_steps=c.td_steps, discount=0.997)
        net = network.MuZeroAtariNet(ATARI_OBS, ATARI_A, 1, 16, 61, 61)
        kw, shape, A = dict(discount=0.997), ATARI_OBS, ATARI_A
        moves = cfg.acc_seq_length + cfg.unroll_steps + cfg.td_steps + 2
        cap = B * cfg.acc_seq_length
        spec = (S, 1, 96, 96, A) if fmt else None
        frames = rs.randint(0, 256, size=(8, B, 1, 96, 96)).astype(np.uint8)
        reset = dict(stack_history=S, is_obs_image=True, frame_shape=(1, 96, 96), frame_u8=True, max_episode_steps=0)
        lens = None
    else:
        B, N = 128, 15
        cfg = types.SimpleNamespace(is_board_game=True, acc_seq_length=9999, unroll_steps=5, td_steps=0, discount=1.0)
        net = network.MuZeroBoardGameNet((9, N, N), N * N + 1, 1, 8)
        kw, shape, A = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0)), (9, N, N), N * N + 1
        moves, cap, spec = (40 if args.quick else 120), 1 << 15, None
        frames = (rs.uniform(size=(8, B, 9, N, N)) < 0.3).astype(np.float32)
        reset = dict(frame_shape=shape, max_episode_steps=64)
        lens = 20 + (np.arange(B) * 7) % 41  # staggered episode lengths, 20 .. 60 moves
    net.load_state_dict(seeded_state_dict(net, 5))
    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=2, num_simulations=1, **kw), 0)
    p.load_state_dict(net.state_dict())
    rp = PrioritizedReplay(cap, 0.0, 0.0, np.random.RandomState(0), device='cuda', **(dict(state_format=fmt, frame_spec=spec) if fmt else {}))
    p.attach_replay(rp, cfg, obs_shape=shape)
    p.selfplay_reset_external(**reset)
    mask, left = np.ones((B, A), np.uint8), None if lens is None else lens.copy()
    per_move, items = [], []
    for m in range(moves):
        p.external_act(frames[m % 8], mask, 1, 2 if lens is not None else 1, 1.0)
        done = np.zeros(B, np.uint8)
        if left is not None:
            left -= 1
            done = (left == 0).astype(np.uint8)
            left[left == 0] = lens[left == 0]
        before = rp.num_added
        p.synchronize()
        p.profile_begin()
        p.external_commit(np.ones(B, np.float32), done)
        per_move.append(p.profile_end()['elapsed_ms'])
        items.append(rp.num_added - before)
    row_bytes = int(np.prod(rp._ring['state'].shape[1:])) * rp._ring['state'].element_size()
    emit = [(t, n) for t, n in zip(per_move, items) if n > 0]
    quiet = sorted(t for t, n in zip(per_move, items) if n == 0)
    top = max(emit, key=lambda x: x[1])
    print(json.dumps(dict(case=args.child, fmt=args.fmt, envs=B, moves=moves, state_row_bytes=row_bytes, items=int(sum(items)),
                          quiet_move_ms_median=quiet[len(quiet) // 2] if quiet else None, emitting_moves=len(emit),
                          emitting_ms_total=sum(t for t, _ in emit), largest_move=dict(items=int(top[1]), ms=top[0], state_bytes_written=int(top[1]) * row_bytes,
                                                                                       state_gb_per_s=int(top[1]) * row_bytes / top[0] / 1e6))))
    p.detach_replay()
    p.close()


def child_gather(args):
    import numpy as np
    import torch

    _, hlm = _setup(args)
    from helpers import seeded_state_dict
    from muzero_amd import network
    from muzero_amd.replay import PrioritizedReplay, Transition

    dev, Bn, K, n = torch.device('cuda', 0), 128, 5, 256
    rs = np.random.RandomState(1)
    if args.fmt == 'frames_u8' or args.net == 'atari':
        net, A, shape = network.MuZeroAtariNet(ATARI_OBS, ATARI_A, 1, 16, 61, 61), ATARI_A, ATARI_OBS
        st = np.concatenate([rs.randint(0, 256, size=(n, S, 96, 96)).astype(np.float32) / 255.0,
                             ((rs.randint(0, A, size=(n, S)) + 1) / A).astype(np.float32)[:, :, None, None] * np.ones((1, 1, 96, 96), np.float32)], axis=1)
        kw = dict(state_format='frames_u8', frame_spec=(S, 1, 96, 96, A)) if args.fmt == 'frames_u8' else {}
    else:
        net, A, shape = network.MuZeroBoardGameNet((9, 15, 15), 226, 1, 8), 226, (9, 15, 15)
        st = (rs.uniform(size=(n,) + shape) < 0.3).astype(np.float32)
        kw = dict(state_format='int8') if args.fmt == 'int8' else {}
    net.load_state_dict(seeded_state_dict(net, 5))
    rp = PrioritizedReplay(n, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw)
    rp.add_batch(Transition(st, rs.randint(0, A, size=(n, K)).astype(np.int16 if A > 128 else np.int8), rs.dirichlet(np.ones(A), size=(n, K)).astype(np.float32),
                            rs.uniform(-1, 1, (n, K)).astype(np.float32), rs.uniform(-1, 1, (n, K)).astype(np.float32)), np.ones(n))
    hl = hlm.HipLearner(net.to(dev), dev, K, Bn, lr=1e-3)
    ring = type(rp._ring)(rp._ring, state=rp._ring['state'].reshape(n, -1))
    idx = torch.from_numpy(rs.randint(0, n, size=Bn).astype(np.int64)).to(dev)
    for _ in range(6):
        hl.grad(ring, idx, None, Bn, frame_spec=kw.get('frame_spec'))
    torch.cuda.synchronize()
    hl.close()


def gather_ns(fmt, net, args):
    """mean duration of k_lc_gather in a rocprofv3 kernel trace of child_gather, first call dropped by taking the minimum and the mean"""
    import csv

    with tempfile.TemporaryDirectory() as d:
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'g', '--', sys.executable, os.path.abspath(__file__), '--child', 'gather', '--fmt', fmt, '--net', net]
        subprocess.run(cmd, check=True, timeout=600, capture_output=True, text=True)
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                if 'k_lc_gather' in row.get('Name', ''):
                    return dict(calls=int(row['Calls']), mean_ns=float(row['AverageNs']), min_ns=float(row['MinNs']), max_ns=float(row['MaxNs']))
    raise RuntimeError('k_lc_gather not found in the kernel trace')


def largest_ring():
    sys.path[:0] = [REPO]
    import numpy as np
    import torch

    from muzero_amd.replay import PrioritizedReplay

    K, A, out = 5, ATARI_A, {}
    shapes = dict(state=ATARI_OBS, action=(K,), pi_prob=(K, A), value=(K,), reward=(K,))
    other = K + 4 * (K * A + 2 * K)
    for fmt, row in (('f32', 294912), ('frames_u8', 36880)):
        free = torch.cuda.mem_get_info(0)[0]
        cap = int(0.9 * free / (row + other))
        kw = dict(state_format=fmt, frame_spec=(S, 1, 96, 96, A)) if fmt != 'f32' else {}
        while True:
            rp = PrioritizedReplay(cap, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw)
            try:
                rp.allocate(shapes)
                break
            except (MemoryError, torch.cuda.OutOfMemoryError):
                cap = int(cap * 0.98)
        out[fmt] = dict(capacity=cap, gib=cap * (row + other) / 2 ** 30, free_gib_before=free / 2 ** 30, over_limit_refused=None)
        try:
            PrioritizedReplay(int(free / (row + other)) + 1, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw).allocate(shapes)
            out[fmt]['over_limit_refused'] = False
        except MemoryError:
            out[fmt]['over_limit_refused'] = True
        del rp
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-planner-lib', default='')
    ap.add_argument('--out-dir', default=os.path.join(REPO, 'profiles', 'replay_codec'))
    ap.add_argument('--quick', action='store_true', help='64 envs and fewer moves: a check of the script, not a measurement')
    ap.add_argument('--skip', default='', help='comma list of legs to skip: atari, gomoku, gather, ring')
    ap.add_argument('--child', default='')
    ap.add_argument('--fmt', default='f32')
    ap.add_argument('--net', default='')
    ap.add_argument('--planner-lib', default='')
    ap.add_argument('--learner-lib', default='')
    a = ap.parse_args()
    if a.child in ('atari', 'gomoku'):
        return child_epilogue(a)
    if a.child == 'gather':
        return child_gather(a)
    os.makedirs(a.out_dir, exist_ok=True)
    skip = set(a.skip.split(','))

    def dump(name, doc):
        with open(os.path.join(a.out_dir, name), 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')
        print(json.dumps(doc, indent=1), flush=True)

    builds = ([('parent_f32', 'f32', a.parent_planner_lib)] if a.parent_planner_lib else [])
    for case, fmt in (('atari', 'frames_u8'), ('gomoku', 'int8')):
        if case in skip:
            continue
        doc = dict(what=__doc__.split('\n\n')[0], quick=a.quick, runs={})
        for name, f, lib in builds + [('this_f32', 'f32', ''), ('this_' + fmt, fmt, '')]:
            doc['runs'][name] = []
            for _ in range(2):
                cmd = [sys.executable, os.path.abspath(__file__), '--child', case, '--fmt', f] + (['--quick'] if a.quick else []) + \
                      (['--planner-lib', os.path.abspath(lib)] if lib else [])
                out = subprocess.run(cmd, check=True, timeout=900, capture_output=True, text=True).stdout
                doc['runs'][name].append(json.loads(out.strip().splitlines()[-1]))
        dump(f'epilogue_{case}.json', doc)
    if 'gather' not in skip:
        doc = dict(what='k_lc_gather at batch 128 (rocprofv3 kernel trace, 6 mzl_grad calls)', rows={})
        for net, fmt in (('atari', 'f32'), ('atari', 'frames_u8'), ('board', 'f32'), ('board', 'int8')):
            try:
                doc['rows'][f'{net}_{fmt}'] = gather_ns(fmt, net, a)
            except Exception as e:  # (the trace tool's output layout differs between ROCm releases)
                doc['rows'][f'{net}_{fmt}'] = dict(error=str(e)[-300:])
        dump('gather.json', doc)
    if 'ring' not in skip:
        dump('largest_ring.json', dict(what='largest capacity PrioritizedReplay.allocate accepts for 8 x 96 x 96 states (K = 5, 18 actions), allocated', **largest_ring()))


if __name__ == '__main__':
    main()
