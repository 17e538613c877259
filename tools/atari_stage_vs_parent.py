#!/usr/bin/env python3
"""Did moving the Atari update's stride-2 loops, pools and entry launch into AtariRun members (for mzl_debug_atari_stage) leave the update alone?  This
tree's library against a built checkout of the parent commit, one MI355X, every leg a fresh child process (a process loads one library):

    python tools/atari_stage_vs_parent.py --parent-tree DIR [--legs 3] [--iters 10] [--skip bench] [--out profiles/atari_stage]

fp32_vs_parent.json   loss, priorities and grad_flat (sha256) after one mzl_grad of a seeded batch: the small Atari net of the tests (batch 5, K = 3) and
                      make_atari_config's size at batch 8.
update_times.json     ms per update (grad + apply) at float32, make_atari_config's size at batch 128 (tools/split_atari_learner_bench.py's leg), parent
                      and this tree alternating; the launches are the same, so this tree's times are to lie within the parent's own spread.
bench_vs_parent.json  bench.py --gpus 1 for both trees alternating and the byte comparison of --dump-outputs per workload."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, os.path.join(REPO, 'tools'))

import split_atari_learner_bench as sab  # noqa: E402


def child_full(B):
    """One mzl_grad at make_atari_config's size, batch B (on whatever library --lib names)."""
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
    tr = sab._atari_batch(rs, B, chan, A, K)
    w = torch.from_numpy(rs.uniform(0.3, 1.0, B).astype(np.float32)).to(dev)
    hl = hlm.HipLearner(net, dev, K, B, lr=1e-3, weight_decay=cfg.weight_decay)
    loss, prio = hl.grad(sab._ring(tr, dev), None, w, B)
    torch.cuda.synchronize()
    print(json.dumps(dict(mode=f'full:{B}', grad_sha256=sab._sha(hl.grad_flat), loss_sha256=sab._sha(loss), priorities_sha256=sab._sha(prio), loss=float(loss))), flush=True)
    hl.close()


def run_child(args, lib=''):
    import subprocess

    cmd = [sys.executable, os.path.abspath(__file__), '--child'] + args + (['--lib', lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit(f'{args} exited with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}')
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--what', default='update', choices=['update', 'default', 'full'])
    ap.add_argument('--lib', default='')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--legs', type=int, default=3)
    ap.add_argument('--parent-tree', default='')
    ap.add_argument('--bench-pairs', type=int, default=1)
    ap.add_argument('--skip', default='', help='comma-separated parts to leave out: bytes, update, bench')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'atari_stage'))
    a = ap.parse_args()
    if a.child:
        if a.lib:
            from muzero_amd import hip_learner as hlm

            hlm.LIB_PATH = a.lib
        return {'update': lambda: sab.child_update('parent', a.iters), 'default': lambda: sab.child_default('atari'), 'full': lambda: child_full(8)}[a.what]()
    if not a.parent_tree:
        sys.exit('--parent-tree: a built checkout of the parent commit')
    skip = set(a.skip.split(','))
    parent_lib = os.path.join(os.path.abspath(a.parent_tree), sab.LIB)
    keys = ('grad_sha256', 'loss_sha256', 'priorities_sha256')
    if 'bytes' not in skip:
        doc = dict(what='the float32 update against the parent commit\'s library, same job: sha256 of grad_flat, loss and priorities after one mzl_grad of a seeded batch')
        for name, what in (('atari_s_batch5', 'default'), ('make_atari_config_batch8', 'full')):
            this, parent = run_child(['--what', what]), run_child(['--what', what], parent_lib)
            doc[name] = dict(this=this, parent=parent, identical=all(this[k] == parent[k] for k in keys))
        doc['all_identical'] = doc['atari_s_batch5']['identical'] and doc['make_atari_config_batch8']['identical']
        sab.dump(os.path.join(a.out, 'fp32_vs_parent.json'), doc)
        print(json.dumps(dict(fp32_vs_parent_all_identical=doc['all_identical'])), flush=True)
    if 'update' not in skip:
        legs = []
        for i in range(a.legs):
            for who, lib in ((('parent', parent_lib), ('this', '')) if i % 2 == 0 else (('this', ''), ('parent', parent_lib))):  # (A B B A ..: no fixed order within a pair)
                leg = run_child(['--what', 'update', '--iters', str(a.iters)], lib)
                leg['mode'] = who
                legs.append(leg)
                print(json.dumps(leg), flush=True)
        upd = dict(what='ms per update (grad + apply) at float32, make_atari_config\'s size at batch 128, wall time over --iters updates after 4 untimed ones; parent and this '
                        'tree alternating (A B B A ..), one fresh process per leg', legs=legs)
        for who in ('parent', 'this'):
            upd[who] = sorted(leg['ms_per_update'] for leg in legs if leg['mode'] == who)
        upd['parent_spread_ms'] = upd['parent'][-1] - upd['parent'][0]
        upd['this_median_minus_parent_median_ms'] = upd['this'][len(upd['this']) // 2] - upd['parent'][len(upd['parent']) // 2]
        upd['this_median_within_parent_range'] = upd['this'][len(upd['this']) // 2] <= upd['parent'][-1]  # (no slower than the parent's own slowest run)
        upd['gradient_identical_to_parent'] = len({leg['grad_sha256'] for leg in legs}) == 1
        sab.dump(os.path.join(a.out, 'update_times.json'), upd)
        print(json.dumps({k: upd[k] for k in ('parent', 'this', 'parent_spread_ms', 'this_median_minus_parent_median_ms', 'this_median_within_parent_range', 'gradient_identical_to_parent')}), flush=True)
    if 'bench' not in skip:
        sab.bench_vs_parent(os.path.abspath(a.parent_tree), a.out, a.bench_pairs)


if __name__ == '__main__':
    main()
