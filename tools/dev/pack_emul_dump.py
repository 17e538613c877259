#!/usr/bin/env python3
"""Writes a conv test net (tests/helpers.py CONV_CASES, or 'board15': 15 x 15, 128 planes, 1 block) as OUT/NAME.txt (config line, then one
line per tensor: name, ndim, dims) + OUT/NAME.bin (float32 values in that order): the input of tools/dev/pack_emul.hip.

    python tools/dev/pack_emul_dump.py NAME OUT"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, REPO)
from helpers import build_conv, conv_case, seeded_state_dict  # noqa: E402
from muzero_amd import network  # noqa: E402

name, out = sys.argv[1], sys.argv[2]
if name == 'board15':
    case = ('board15', 'board', (9, 15, 15), 226, 1, 128, 1, 1, 31)
    net = network.MuZeroBoardGameNet((9, 15, 15), 226, 1, 128)
    net.load_state_dict(seeded_state_dict(net, 31))
else:
    case = conv_case(name)
    net = build_conv(case)
_, kind, ishape, A, R, P, vs, rs, _ = case
os.makedirs(out, exist_ok=True)
with open(os.path.join(out, name + '.txt'), 'w') as f, open(os.path.join(out, name + '.bin'), 'wb') as b:
    f.write(f'{1 if kind == "board" else 2} {ishape[0]} {ishape[1]} {ishape[2]} {A} {R} {P} {vs} {rs}\n')
    for k, v in net.state_dict().items():
        if k.endswith('num_batches_tracked'):
            continue
        a = v.numpy().astype(np.float32)
        f.write(k + ' ' + str(a.ndim) + ' ' + ' '.join(map(str, a.shape)) + '\n')
        b.write(a.tobytes())
