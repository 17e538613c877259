#!/usr/bin/env python3
"""The Atari learner's opt-in split-bf16 convs (HipLearner(tower_precision=, stage_precision=), mzl_set_atari_precision) against the float32 update, at
make_atari_config's size (96 x 96 frames, 128 planes, 8 blocks, K = 5, batch 128, seeded random weights and batch), on one MI355X.  Every leg is a
fresh child process; legs alternate.  Writes profiles/split_atari_learner/*.json:

    python tools/split_atari_learner_bench.py [--legs 2] [--iters 10] [--parent-tree DIR] [--out profiles/split_atari_learner]

update_times.json   ms per update (grad + apply, wall time over --iters updates after 3 untimed ones) for the four combinations of
                    tower_precision / stage_precision, and -- with --parent-tree, a built checkout of the parent commit -- for the parent's library.
launch_times.json   HIP-event time of ONE conv launch, float32 against split, 128 -> 128 channels at batch 128: a 6 x 6 and a 12 x 12 whole-image conv
                    (mzl_debug_conv on a board handle: the towers' tilings, identity staging, unpaired) and a 24 x 24 and a 48 x 48 tile-path conv
                    (mzl_debug_conv_tile: the update's gather, op builder and dispatcher); median of 5 calls after an untimed one.
accuracy.json       the tile-path conv's error against float64 relative to a sequential float32 chain's (tests/test_gpu_split_atari_learner.py).
fp32_vs_parent.json the gradient vector (sha256) of the default Atari handle and of a board handle at both conv_precision values, this library
                    against the parent's.
bench_vs_parent.json  bench.py --gpus 1 (headline and learner legs) for this tree and the parent's alternating, and the byte comparison of
                    --dump-outputs per workload."""
import argparse
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

BATCH = 128
COMBOS = ('f32/f32', 'bf16x3/f32', 'f32/bf16x3', 'bf16x3/bf16x3')  # tower_precision / stage_precision
LIB = os.path.join('muzero_amd', 'lib', 'libmzlearner_hip.so')


def _atari_batch(rs, B, chan, A, K):
    import numpy as np

    from muzero_amd.replay import Transition

    return Transition(rs.uniform(0, 1, (B, chan, 96, 96)).astype(np.float32), rs.randint(0, A, (B, K)).astype(np.int8),
                      rs.dirichlet(np.ones(A), size=(B, K)).astype(np.float32), (rs.uniform(-1, 1, (B, K)) * 8.0).astype(np.float32),
                      rs.uniform(-1, 1, (B, K)).astype(np.float32))


def _ring(tr, dev):
    import torch

    B = tr.state.shape[0]
    return dict(state=torch.from_numpy(tr.state).to(dev).reshape(B, -1).contiguous(), action=torch.from_numpy(tr.action).to(dev),
                pi_prob=torch.from_numpy(tr.pi_prob).to(dev), value=torch.from_numpy(tr.value).to(dev), reward=torch.from_numpy(tr.reward).to(dev))


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def child_update(mode, iters):
    import numpy as np
    import torch

    from helpers import seeded_state_dict
    from muzero_amd import hip_learner as hlm
    from muzero_amd.config import make_atari_config
    from muzero_amd.network import MuZeroAtariNet

    dev = torch.device('cuda', 0)
    cfg = make_atari_config(use_tensorboard=False)
    K, chan, A = cfg.unroll_steps, 4, 6
    net = MuZeroAtariNet((chan, 96, 96), A, cfg.num_res_blocks, cfg.num_planes, cfg.value_support_size, cfg.reward_support_size)
    net.load_state_dict(seeded_state_dict(net, 211))
    net = net.to(dev)
    rs = np.random.RandomState(8)
    tr = _atari_batch(rs, BATCH, chan, A, K)
    ring = _ring(tr, dev)
    w = torch.from_numpy(rs.uniform(0.3, 1.0, BATCH).astype(np.float32)).to(dev)
    kw = {} if mode == 'parent' else dict(zip(('tower_precision', 'stage_precision'), mode.split('/')))
    hl = hlm.HipLearner(net, dev, K, BATCH, lr=1e-3, weight_decay=cfg.weight_decay, **kw)
    hl.grad(ring, None, w, BATCH)
    torch.cuda.synchronize()
    res = dict(mode=mode, net=f'MuZeroAtariNet {chan}x96x96, {cfg.num_planes} planes, {cfg.num_res_blocks} blocks, A={A}', batch=BATCH, unroll=K, iters=iters,
               grad_sha256=_sha(hl.grad_flat), loss=float(hl.loss))

    def step():
        hl.grad(ring, None, w, BATCH)
        hl.apply()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    res['ms_per_update'] = 1e3 * (time.perf_counter() - t0) / iters
    hl.close()
    print(json.dumps(res), flush=True)


def child_launch():
    import numpy as np
    import torch

    from helpers import build_conv, conv_case
    from muzero_amd import hip_learner as hlm

    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(3)
    C_ = 128
    wt = (rs.randn(C_, C_, 3, 3) * 0.05).astype(np.float32)
    res = {}

    def median_us(call):
        us = []
        for _ in range(6):
            _, name = call()
            us.append(float(name.rsplit('us=', 1)[1]))
        return dict(build=name.rsplit(' us=', 1)[0], us_median=sorted(us[1:])[2], us_all=us)

    atari = hlm.HipLearner(build_conv(conv_case('atari_s')).to(dev), dev, 1, 2, lr=1e-3)
    for key, side in (('tile_24x24', 24), ('tile_48x48_wide', 48)):
        x = rs.uniform(0, 1, (BATCH, C_, side, side)).astype(np.float32)
        res[key] = {p: median_us(lambda p=p: atari.debug_conv_tile(0, wt, x, precision=p)) for p in ('f32', 'bf16x3')}
    atari.close()
    for p in ('f32', 'bf16x3'):
        board = hlm.HipLearner(build_conv(conv_case('board3')).to(dev), dev, 5, 4, lr=1e-3, conv_precision=p)
        for key, side in (('tower_6x6', 6), ('stage_12x12', 12)):
            x = rs.uniform(0, 1, (BATCH, C_, side, side)).astype(np.float32)
            res.setdefault(key, {})[p] = median_us(lambda: board.debug_conv(0, wt, x))
        board.close()
    for v in res.values():
        v['speedup_bf16x3_over_f32'] = v['f32']['us_median'] / v['bf16x3']['us_median']
    print(json.dumps(res), flush=True)


def child_default(mode):
    """The gradient vector of a default-path handle: atari | board:f32 | board:bf16x3 (on whatever library --lib names)."""
    import numpy as np
    import torch

    from helpers import build_conv, conv_case
    from muzero_amd import hip_learner as hlm
    from test_gpu_conv_learner import _batch, _net

    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(17)
    if mode == 'atari':
        net, B, K = build_conv(conv_case('atari_s')).to(dev), 5, 3
        tr = _atari_batch(rs, B, 4, 6, K)
        kw = {}
    else:
        B, K = 6, 5
        net, A = _net(9, 32, 2, 4, 91, dev)
        tr = _batch(rs, B, (4, 9, 9), A)
        kw = dict(conv_precision=mode.split(':')[1])
    w = torch.from_numpy(rs.uniform(0.3, 1.0, B).astype(np.float32)).to(dev)
    hl = hlm.HipLearner(net, dev, K, B, lr=1e-3, **kw)
    loss, prio = hl.grad(_ring(tr, dev), None, w, B)
    torch.cuda.synchronize()
    print(json.dumps(dict(mode=mode, grad_sha256=_sha(hl.grad_flat), loss_sha256=_sha(loss), priorities_sha256=_sha(prio), loss=float(loss))), flush=True)
    hl.close()


def child_accuracy():
    import numpy as np
    import torch

    import split_atari_cases as sa
    from helpers import build_conv, conv_case
    from muzero_amd import hip_learner as hlm
    from test_gpu_split_atari_learner import BAR, tile_accuracy

    dev = torch.device('cuda', 0)
    hl = hlm.HipLearner(build_conv(conv_case('atari_s')).to(dev), dev, 1, 2, lr=1e-3)
    out = dict(what='one tile-path conv (48 -> 24 channels, batch 2) through mzl_debug_conv_tile: rel. rms error against float64 divided by a sequential float32 chain\'s, '
                    'over the whole output and per output channel', bar=BAR, cases=[])
    for plane in sa.PLANES:
        for direction in (0, 1):
            for p in ('f32', 'bf16x3'):
                res, name = tile_accuracy(hl, plane, direction, p)
                out['cases'].append(dict(plane=plane, direction='dgrad' if direction else 'forward', precision=p, build=name.rsplit(' us=', 1)[0],
                                         whole_ratio=float(res['whole'][0].max()), channel_ratio_max=float(res['channel'][0].max()),
                                         channel_ratio_median=float(np.median(res['channel'][0])), kernel_error_whole=float(res['whole'][1].max()),
                                         chain32_error_whole=float(res['whole'][2].max())))
    out['worst_ratio'] = max(max(c['whole_ratio'], c['channel_ratio_max']) for c in out['cases'])
    hl.close()
    print(json.dumps(out), flush=True)


def run_child(args, lib=''):
    cmd = [sys.executable, os.path.abspath(__file__), '--child'] + args + (['--lib', lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f'{args} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


def dump(path, doc):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


def bench_vs_parent(parent_tree, out, pairs):
    """bench.py in both trees, alternating (headline + learner legs), then --dump-outputs per workload, compared byte for byte."""
    import numpy as np

    def bench(tree, extra):
        r = subprocess.run([sys.executable, 'bench.py', '--gpus', '1'] + extra, cwd=tree, capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            sys.exit(f'bench.py in {tree} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
        return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])

    legs = ['--steps', '30', '--warmup', '5', '--no-cpu-baseline', '--no-sustained', '--no-e2e', '--no-configs']
    doc = {}
    for i in range(1, pairs + 1):
        for name, tree in (('new', REPO), ('parent', parent_tree)):
            r = bench(tree, legs)
            doc[f'{name}_{i}'] = dict(value=r.get('value'), ms_per_step=r.get('ms_per_step'), metric=r.get('metric'), learner=r.get('learner'))
            print(json.dumps({f'{name}_{i}': doc[f'{name}_{i}']}), flush=True)
    doc['dump_outputs'] = {}
    for wl in ('c2', 'c3', 'c5', 'lunar'):
        with tempfile.TemporaryDirectory() as da, tempfile.TemporaryDirectory() as db:
            for tree, d in ((REPO, da), (parent_tree, db)):
                bench(tree, ['--steps', '3', '--warmup', '1', '--workload', wl, '--dump-outputs', d, '--no-cpu-baseline', '--no-sustained', '--no-e2e', '--no-configs',
                             '--no-learner'])
            same = total = 0
            for root, _, files in os.walk(da):
                for f in sorted(files):
                    pa = os.path.join(root, f)
                    pb = os.path.join(db, os.path.relpath(pa, da))
                    if f.endswith('.npz'):
                        a, b = np.load(pa), np.load(pb)
                        for k in a.files:
                            total += 1
                            same += int(k in b.files and a[k].tobytes() == b[k].tobytes())
                    else:
                        total += 1
                        same += int(os.path.exists(pb) and open(pa, 'rb').read() == open(pb, 'rb').read())
            doc['dump_outputs'][wl] = f'{"identical to" if same == total and total else "DIFFERENT from"} the parent commit, {same} of {total} arrays byte for byte'
    doc['_note'] = ('one job on one MI355X: bench.py --gpus 1 --steps 30 --warmup 5 (headline and learner legs) for this commit / the parent alternating, then '
                    '--dump-outputs (--steps 3 --warmup 1) per workload for both')
    dump(os.path.join(out, 'bench_vs_parent.json'), doc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--what', default='update', choices=['update', 'launch', 'default', 'accuracy'])
    ap.add_argument('--mode', default='f32/f32')
    ap.add_argument('--lib', default='')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--legs', type=int, default=2)
    ap.add_argument('--parent-tree', default='')
    ap.add_argument('--bench-pairs', type=int, default=2)
    ap.add_argument('--skip', default='', help='comma-separated parts to leave out: update, launch, accuracy, default, bench')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'split_atari_learner'))
    a = ap.parse_args()
    if a.child:
        if a.lib:
            from muzero_amd import hip_learner as hlm

            hlm.LIB_PATH = a.lib
        return {'update': lambda: child_update(a.mode, a.iters), 'launch': child_launch, 'default': lambda: child_default(a.mode), 'accuracy': child_accuracy}[a.what]()
    skip = set(a.skip.split(','))
    parent_lib = os.path.join(os.path.abspath(a.parent_tree), LIB) if a.parent_tree else ''
    if 'update' not in skip:
        modes = (['parent'] if parent_lib else []) + list(COMBOS)
        legs = []
        for _ in range(a.legs):
            for mode in modes:
                legs.append(run_child(['--what', 'update', '--mode', mode, '--iters', str(a.iters)], parent_lib if mode == 'parent' else ''))
                print(json.dumps(legs[-1]), flush=True)
        upd = dict(legs=legs)
        for mode in modes:
            upd[mode] = sorted(leg['ms_per_update'] for leg in legs if leg['mode'] == mode)
        upd['spread_ms_max'] = max(upd[m][-1] - upd[m][0] for m in modes)
        for m in COMBOS[1:]:
            upd['speedup_' + m.replace('/', '_') + '_over_f32'] = upd['f32/f32'][0] / upd[m][0]
        if parent_lib:
            shas = {m: sorted({leg['grad_sha256'] for leg in legs if leg['mode'] == m}) for m in ('parent', 'f32/f32')}
            upd['default_gradient_identical_to_parent'] = shas['parent'] == shas['f32/f32'] and len(shas['parent']) == 1
        dump(os.path.join(a.out, 'update_times.json'), upd)
    if 'launch' not in skip:
        lt = run_child(['--what', 'launch'])
        lt['what'] = 'HIP events around ONE forward conv launch, 128 -> 128 channels, batch 128; median of 5 calls after an untimed one'
        dump(os.path.join(a.out, 'launch_times.json'), lt)
        print(json.dumps({k: v.get('speedup_bf16x3_over_f32') for k, v in lt.items() if isinstance(v, dict)}), flush=True)
    if 'accuracy' not in skip:
        acc = run_child(['--what', 'accuracy'])
        dump(os.path.join(a.out, 'accuracy.json'), acc)
        print(json.dumps(dict(worst_ratio=acc['worst_ratio'])), flush=True)
    if 'default' not in skip and parent_lib:
        doc = dict(what='the default paths against the parent commit\'s library, same job: sha256 of the gradient vector, loss and priorities of one fixed batch')
        for mode in ('atari', 'board:f32', 'board:bf16x3'):
            this, parent = run_child(['--what', 'default', '--mode', mode]), run_child(['--what', 'default', '--mode', mode], parent_lib)
            doc[mode] = dict(this=this, parent=parent, identical=all(this[k] == parent[k] for k in ('grad_sha256', 'loss_sha256', 'priorities_sha256')))
        doc['all_identical'] = all(doc[m]['identical'] for m in ('atari', 'board:f32', 'board:bf16x3'))
        dump(os.path.join(a.out, 'fp32_vs_parent.json'), doc)
        print(json.dumps(dict(fp32_vs_parent_all_identical=doc['all_identical'])), flush=True)
    if 'bench' not in skip and a.parent_tree:
        bench_vs_parent(os.path.abspath(a.parent_tree), a.out, a.bench_pairs)


if __name__ == '__main__':
    main()
