"""Are the learner's gradient vector, loss and priorities the same bytes as another build's?  The diagnostic hook mzl_debug_wgrad reaches into the update's op builders
(Sched::wgrad_ops, wgrad_ops_steps, AtariRun::wgrad_tiles were given parameters and split for it) and make_geom; the update itself must not move.

    python tools/wgrad_vs_parent.py --parent-lib PATH/libmzlearner_hip.so [--out profiles/wgrad_layer/fp32_vs_parent.json]

One child process per library and case (a process loads one library): sha256 of grad_flat after one mzl_grad of a fixed batch, for two geometries
of tests/test_gpu_conv_learner.py -- (9, 32 planes, 3 blocks, batch 64): 82 action planes on the sparse route; (15, 32 planes, 2 blocks, batch 10):
the 15 x 15 builds -- and the small Atari case of tests/test_gpu_atari_learner.py."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {'board9_p32_r3_n64': ('board', (9, 32, 3, 9, 64, True)), 'board15_p32_r2_n10': ('board', (15, 32, 2, 9, 10, True)),
         'atari_p8_r1_n3': ('atari', (4, 8, 1, 6, 11, 11, 3, 5, 3))}


def child(case, lib):
    sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
    import numpy as np
    import torch

    from muzero_amd import hip_learner as hlm
    if lib:
        hlm.LIB_PATH = lib
    dev = torch.device('cuda', 0)
    kind, g = CASES[case]
    if kind == 'board':
        from test_gpu_conv_learner import _batch, _hip, _net, _ring
        board, planes, blocks, chan, B, int8_state = g
        net, A = _net(board, planes, blocks, chan, 100 + board, dev)
        net.train()
        rs = np.random.RandomState(board * 7 + B)
        tr = _batch(rs, B, (chan, board, board), A, int8_state=int8_state)
        K = 5
    else:
        from helpers import seeded_state_dict
        from muzero_amd.network import MuZeroAtariNet
        from muzero_amd.replay import Transition
        from test_gpu_atari_learner import _hip, _ring
        chan, planes, blocks, A, vs, rs_, B, K, seed = g
        net = MuZeroAtariNet((chan, 96, 96), A, blocks, planes, vs, rs_)
        net.load_state_dict(seeded_state_dict(net, 100 + seed))
        net = net.to(dev)
        net.train()
        rs = np.random.RandomState(seed)
        tr = Transition(rs.uniform(0, 1, (B, chan, 96, 96)).astype(np.float32), rs.randint(0, A, (B, K)).astype(np.int8),
                        rs.dirichlet(np.ones(A), size=(B, K)).astype(np.float32), (rs.uniform(-1, 1, (B, K)) * 8.0).astype(np.float32),
                        rs.uniform(-1, 1, (B, K)).astype(np.float32))
    w = rs.uniform(0.3, 1.0, B).astype(np.float32)
    hl = _hip(net, dev, B, K=K)
    loss, prio = hl.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    g = hl.grad_flat.detach().cpu().numpy()
    print(json.dumps(dict(case=case, sha256=hashlib.sha256(g.tobytes()).hexdigest(), floats=int(g.size), loss=float(loss),
                          loss_bits=loss.detach().cpu().numpy().tobytes().hex(), priorities_sha256=hashlib.sha256(prio.detach().cpu().numpy().tobytes()).hexdigest())))
    hl.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', default='')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'wgrad_layer', 'fp32_vs_parent.json'))
    ap.add_argument('--child', default='')
    ap.add_argument('--lib', default='')
    a = ap.parse_args()
    if a.child:
        child(a.child, a.lib)
        sys.exit(0)
    doc = dict(what='sha256 of the gradient vector (grad_flat), the bits of the loss and sha256 of the priorities after one mzl_grad of a fixed batch: this tree\'s library against the parent '
                    'commit\'s, same job', cases={})
    for case in CASES:
        row = {}
        for who, lib in (('parent', os.path.abspath(a.parent_lib)), ('this', '')):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', case, '--lib', lib], check=True, timeout=300, capture_output=True, text=True).stdout
            row[who] = json.loads(out.strip().splitlines()[-1])
        same = all(row['parent'][k] == row['this'][k] for k in ('sha256', 'floats', 'loss_bits', 'priorities_sha256'))
        doc['cases'][case] = dict(parent=row['parent']['sha256'], this=row['this']['sha256'], floats=row['this']['floats'], loss_bits=[row['parent']['loss_bits'], row['this']['loss_bits']],
                                  priorities=[row['parent']['priorities_sha256'], row['this']['priorities_sha256']], identical=same)
    doc['identical'] = all(c['identical'] for c in doc['cases'].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print(json.dumps(doc, indent=1))
    sys.exit(0 if doc['identical'] else 1)
