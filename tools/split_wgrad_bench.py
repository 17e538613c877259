#!/usr/bin/env python3
"""The board-net learner's split-bf16 weight gradient (HipLearner(wgrad_precision='bf16x3'), csrc/mz_learn_conv_split_wgrad.h) against the float32
kernel, on C5's net (15 x 15, 128 planes, 8 blocks, K = 5, batch 128, seeded random weights and batch).  Every leg is a fresh child process; legs
alternate.

    python tools/split_wgrad_bench.py [--legs 2] [--iters 20] [--parent-lib PATH/libmzlearner_hip.so] [--out profiles/split_wgrad]

Per launch (launch_times.json): the paired 128 -> 128 weight gradient of the towers (two layers in one launch, the update's own chunking) through
the library's diagnostic hook, which brackets the kernel with HIP events; median of 5 calls after an untimed one, float32 kernel and split kernel.
Per update (update_times.json): ms per update (grad + apply, wall time over --iters updates after 3 untimed ones) for the four combinations of
conv_precision x wgrad_precision, and the sha256 of the gradient vector of one fixed batch.  --parent-lib: the default path on the parent commit's
library in the same job (`parent`): its times beside this tree's default-wgrad legs, and the byte comparison of the gradient."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

BOARD, PLANES, BLOCKS, CHAN, BATCH = 15, 128, 8, 9, 128
COMBOS = ('f32/f32', 'f32/bf16x3', 'bf16x3/f32', 'bf16x3/bf16x3')  # conv_precision / wgrad_precision


def child(mode, lib, iters):
    import numpy as np
    import torch

    from muzero_amd import hip_learner as hlm
    from muzero_amd.config import make_gomoku_config
    from test_gpu_conv_learner import _batch, _net, _ring

    if lib:
        hlm.LIB_PATH = lib
    dev = torch.device('cuda', 0)
    cfg = make_gomoku_config(use_tensorboard=False)
    K = cfg.unroll_steps
    net, A = _net(BOARD, PLANES, BLOCKS, CHAN, 177, dev)
    rs = np.random.RandomState(6)
    tr = _batch(rs, BATCH, (CHAN, BOARD, BOARD), A, K=K, int8_state=True)
    ring = _ring(tr, dev)
    w = torch.from_numpy(rs.uniform(0.3, 1.0, BATCH).astype(np.float32)).to(dev)
    kw = {} if mode == 'parent' else dict(zip(('conv_precision', 'wgrad_precision'), mode.split('/')))
    hl = hlm.HipLearner(net, dev, K, BATCH, lr=cfg.lr_init, weight_decay=cfg.weight_decay, **kw)
    hl.grad(ring, None, w, BATCH)
    torch.cuda.synchronize()
    res = dict(mode=mode, net=f'MuZeroBoardGameNet {BOARD}x{BOARD}, {PLANES} planes, {BLOCKS} blocks, A={A}', batch=BATCH, unroll=K, iters=iters,
               grad_sha256=hashlib.sha256(hl.grad_flat.cpu().numpy().tobytes()).hexdigest(), loss=float(hl.loss))

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
    if mode in ('f32/f32', 'f32/bf16x3'):  # the towers' paired weight-gradient launch
        x = rs.uniform(0, 1, (2, BATCH, PLANES, BOARD, BOARD)).astype(np.float32)
        dz = (rs.randn(2, BATCH, PLANES, BOARD, BOARD) * 0.05).astype(np.float32)
        us = []
        for _ in range(6):
            _, name = hl.debug_wgrad(dz[0], x[0], mode='pair', second=dict(dz=dz[1], x=x[1]))
            us.append(float(name.rsplit('us=', 1)[1]))
        res['wgrad_pair'] = dict(build=name.rsplit(' us=', 1)[0], us_median=sorted(us[1:])[2], us_all=us)
    hl.close()
    print(json.dumps(res), flush=True)


def run_child(mode, lib, iters):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--mode', mode, '--iters', str(iters)] + (['--lib', lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f'{mode} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


def dump(path, doc):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--mode', default='f32/f32')
    ap.add_argument('--lib', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--legs', type=int, default=2)
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'split_wgrad'))
    a = ap.parse_args()
    if a.child:
        return child(a.mode, a.lib, a.iters)
    modes = (['parent'] if a.parent_lib else []) + list(COMBOS)
    legs = []
    for _ in range(a.legs):
        for mode in modes:
            legs.append(run_child(mode, os.path.abspath(a.parent_lib) if mode == 'parent' else '', a.iters))
            print(json.dumps(legs[-1]), flush=True)
    upd = dict(legs=[{k: v for k, v in leg.items() if k != 'wgrad_pair'} for leg in legs])
    for mode in modes:
        upd[mode] = sorted(leg['ms_per_update'] for leg in legs if leg['mode'] == mode)
    spread = max(upd[m][-1] - upd[m][0] for m in modes)
    upd['spread_ms_max'] = spread
    upd['speedup_wgrad_bf16x3_at_conv_f32'] = upd['f32/f32'][0] / upd['f32/bf16x3'][0]
    upd['speedup_wgrad_bf16x3_at_conv_bf16x3'] = upd['bf16x3/f32'][0] / upd['bf16x3/bf16x3'][0]
    dump(os.path.join(a.out, 'update_times.json'), upd)
    lt = {m: dict(build=[leg['wgrad_pair']['build'] for leg in legs if leg['mode'] == m][0],
                  us_median=sorted(leg['wgrad_pair']['us_median'] for leg in legs if leg['mode'] == m),
                  us_all=[leg['wgrad_pair']['us_all'] for leg in legs if leg['mode'] == m]) for m in ('f32/f32', 'f32/bf16x3')}
    f, s = lt['f32/f32']['us_median'], lt['f32/bf16x3']['us_median']
    lt['what'] = 'the paired 128 -> 128 weight-gradient launch of the C5 towers (15 x 15, batch 128), HIP events around the kernel; one median per leg'
    lt['spread_us'] = max(f[-1] - f[0], s[-1] - s[0])
    lt['speedup_bf16x3_over_f32'] = f[0] / s[0]
    lt['split_is_faster_by_more_than_the_spread'] = bool(f[0] - s[-1] > lt['spread_us'])
    dump(os.path.join(a.out, 'launch_times.json'), lt)
    if a.parent_lib:
        shas = {m: sorted({leg['grad_sha256'] for leg in legs if leg['mode'] == m}) for m in ('parent', 'f32/f32')}
        dump(os.path.join(a.out, 'default_vs_parent.json'),
             dict(what='the default path (conv f32, wgrad f32) against the parent commit\'s library, same job: sha256 of the gradient vector of one fixed batch, ms per update',
                  parent=shas['parent'], this=shas['f32/f32'], identical=shas['parent'] == shas['f32/f32'] and len(shas['f32/f32']) == 1,
                  ms_per_update=dict(parent=upd['parent'], this_f32_f32=upd['f32/f32'], this_bf16x3_f32=upd['bf16x3/f32']), spread_ms_max=spread))
    print(json.dumps({k: v for k, v in upd.items() if k != 'legs'}), flush=True)
    print(json.dumps({k: v for k, v in lt.items() if k not in ('f32/f32', 'f32/bf16x3')}), flush=True)


if __name__ == '__main__':
    main()
