#!/usr/bin/env python3
"""The board-net learner's split-bf16 convs (HipLearner(conv_precision='bf16x3'), csrc/mz_learn_conv_split.h) against its float32 path: C5's net
(15 x 15, 128 planes, 8 blocks, K = 5, batch 128, seeded random weights and batch).  Every leg is a fresh child process; legs alternate.

    python tools/split_learner_bench.py [--legs 2] [--parent-lib PATH/libmzlearner_hip.so] [--out profiles/split_learner]
    python tools/split_learner_bench.py --accuracy [--out profiles/split_learner]

Per leg: ms per update (grad + apply, wall time over --iters updates after 3 untimed ones), one forward and one data-gradient conv launch of the
towers' layer shape (128 -> 128 at batch 128) through the library's diagnostic hook, which brackets its launch with HIP events (identity staging, no
statistics; median of 5 calls after an untimed one), and the sha256 of the gradient vector of one fixed batch.  --parent-lib: the same float32 legs
on the parent commit's library in the same job (`f32-parent`; it has no hook, so no launch times): update_times.json holds all legs,
fp32_vs_parent.json the byte comparison of the default path's gradient with the parent's.
--accuracy: per geometry of tests/test_gpu_conv_learner.py and per gradient tensor, the split learner's and the f32 learner's error against float64
autograd on the pass's own branch and their ratio, as tests/test_gpu_split_learner.py measures them -> accuracy.json."""
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


def child(mode, lib, iters):
    import numpy as np
    import torch

    from muzero_amd import build as mz_build
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
    kw = {} if mode == 'f32-parent' else dict(conv_precision=mode)
    hl = hlm.HipLearner(net, dev, K, BATCH, lr=cfg.lr_init, weight_decay=cfg.weight_decay, **kw)
    hl.grad(ring, None, w, BATCH)
    torch.cuda.synchronize()
    res = dict(mode=mode, net=f'MuZeroBoardGameNet {BOARD}x{BOARD}, {PLANES} planes, {BLOCKS} blocks, A={A}', batch=BATCH, unroll=K, iters=iters,
               grad_sha256=hashlib.sha256(hl.grad_flat.cpu().numpy().tobytes()).hexdigest(), loss=float(hl.loss),
               _learner_fingerprint=None if lib else mz_build.learner_fingerprint())

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
    res['tflops'] = hlm.conv_learner_flops((CHAN, BOARD, BOARD), A, BLOCKS, PLANES, K) * BATCH / (res['ms_per_update'] * 1e-3) / 1e12
    if mode != 'f32-parent':
        wt = (rs.randn(PLANES, PLANES, 3, 3) * 0.05).astype(np.float32)
        x = rs.uniform(0, 1, (BATCH, PLANES, BOARD, BOARD)).astype(np.float32)
        for direction, key in ((0, 'forward'), (1, 'dgrad')):
            us = []
            for _ in range(6):
                _, name = hl.debug_conv(direction, wt, x)
                us.append(float(name.rsplit('us=', 1)[1]))
            res[f'conv_{key}'] = dict(build=name.rsplit(' us=', 1)[0], us_median=sorted(us[1:])[2], us_all=us)
    hl.close()
    print(json.dumps(res), flush=True)


def run_child(mode, lib, iters):
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--mode', mode, '--iters', str(iters)] + (['--lib', lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit(f'{mode} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


def accuracy(out):
    import torch

    from test_gpu_conv_learner import GEOMETRIES, same_branch_bar
    from test_gpu_split_learner import split_vs_f32_errors, worst_against_bar

    dev = torch.device('cuda', 0)
    doc = {'statistic': 'max |g - g64| / max |g64| per gradient tensor, float64 autograd on the pass\'s own branch (tests/forced_masks.py); ratio = bf16x3 / f32',
           'bar': 'max(same_branch_bar, 2 x the f32 HIP learner\'s error of the tensor)', 'geometries': {}}
    for board, planes, blocks, chan, B, int8_state in GEOMETRIES:
        r = split_vs_f32_errors(board, planes, blocks, chan, B, int8_state, dev)
        r['hl'].close()
        k, e, bar, second = worst_against_bar(r)
        ratios = {t: (r['errs'][t] / r['e32'][t] if r['e32'][t] > 0 else None) for t in r['errs']}
        finite = [v for v in ratios.values() if v is not None]
        doc['geometries'][f'b{board}-p{planes}-r{blocks}-n{B}'] = dict(
            worst_tensor=k, worst_error=float('%.4g' % e), worst_bar=float('%.4g' % bar), flat_bar=float('%.4g' % same_branch_bar(r['errs'], r['err_t32'])[2]),
            passes=bool(e <= bar), passes_through_second_term_only=bool(second and e <= bar), ratio_max=float('%.4g' % max(finite)),
            ratio_median=float('%.4g' % sorted(finite)[len(finite) // 2]),
            tensors={t: dict(bf16x3=float('%.4g' % r['errs'][t]), f32=float('%.4g' % r['e32'][t]), ratio=None if ratios[t] is None else float('%.4g' % ratios[t]))
                     for t in r['errs']})
        print(json.dumps({kk: v for kk, v in doc['geometries'][f'b{board}-p{planes}-r{blocks}-n{B}'].items() if kk != 'tensors'}), flush=True)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, 'accuracy.json'), 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--mode', default='f32')
    ap.add_argument('--lib', default='')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--legs', type=int, default=2)
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--accuracy', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'split_learner'))
    a = ap.parse_args()
    if a.child:
        return child(a.mode, a.lib, a.iters)
    if a.accuracy:
        return accuracy(a.out)
    modes = (['f32-parent'] if a.parent_lib else []) + ['f32', 'bf16x3']
    legs = []
    for _ in range(a.legs):
        for mode in modes:
            legs.append(run_child(mode, a.parent_lib if mode == 'f32-parent' else '', a.iters))
            print(json.dumps(legs[-1]), flush=True)
    summary = dict(legs=legs)
    for mode in modes:
        ms = sorted(leg['ms_per_update'] for leg in legs if leg['mode'] == mode)
        summary[mode] = dict(ms_per_update_min=ms[0], ms_per_update_max=ms[-1])
        for key in ('conv_forward', 'conv_dgrad'):
            us = sorted(leg[key]['us_median'] for leg in legs if leg['mode'] == mode and key in leg)
            if us:
                summary[mode][key + '_us'] = us
    summary['speedup_bf16x3_over_f32'] = summary['f32']['ms_per_update_min'] / summary['bf16x3']['ms_per_update_min']
    summary['f32_spread_ms'] = summary['f32']['ms_per_update_max'] - summary['f32']['ms_per_update_min']
    for key in ('conv_forward', 'conv_dgrad'):
        summary[f'speedup_{key}'] = min(summary['f32'][key + '_us']) / min(summary['bf16x3'][key + '_us'])
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'update_times.json'), 'w') as f:
        json.dump(summary, f, indent=1)
        f.write('\n')
    if a.parent_lib:
        shas = {m: sorted({leg['grad_sha256'] for leg in legs if leg['mode'] == m}) for m in ('f32-parent', 'f32')}
        cmp_doc = dict(what='sha256 of the gradient vector (grad_flat) of one fixed batch, C5 net at batch 128: the default path against the parent commit\'s library, same job',
                       parent=shas['f32-parent'], this=shas['f32'], identical=shas['f32-parent'] == shas['f32'] and len(shas['f32']) == 1,
                       ms_per_update=dict(parent=sorted(leg['ms_per_update'] for leg in legs if leg['mode'] == 'f32-parent'),
                                          this=sorted(leg['ms_per_update'] for leg in legs if leg['mode'] == 'f32')))
        with open(os.path.join(a.out, 'fp32_vs_parent.json'), 'w') as f:
            json.dump(cmp_doc, f, indent=1)
            f.write('\n')
    print(json.dumps({k: v for k, v in summary.items() if k != 'legs'}), flush=True)


if __name__ == '__main__':
    main()
