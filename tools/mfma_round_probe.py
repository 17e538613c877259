"""How one v_mfma_f32_16x16x32_bf16 rounds, seen through the split-bf16 conv (Planner.debug_conv3x3, conv_precision='bf16x3').

    python tools/mfma_round_probe.py > profiles/conv_layer/mfma_rounding.txt      (one MI355X)

A 3 x 3 image of ones, 32 input channels, centre-tap weights of 1 on the k slots named in each row (-1 where the bias is negative) and
a bias of +-2^24 .. +-2^31 per output channel: the centre output is bias + n in exact arithmetic, and only the hh MFMA of the centre tap
adds anything but zeros.  What comes back tells how many of the n ones the instruction summed before it rounded them into the
accumulator.  The float32 kernel (one fmaf per product) loses every one of them: the last rows."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
from helpers import build_conv, conv_case  # noqa: E402
from muzero_amd import planner as pl  # noqa: E402

ROWS = {
    'k 0..31': list(range(32)), 'k 0..15': list(range(16)), 'k 0..7': list(range(8)), 'k 0..3': [0, 1, 2, 3], 'k 0,1': [0, 1], 'k 0': [0],
    'k 0,1,2': [0, 1, 2], 'k 0,4': [0, 4], 'k 0,8': [0, 8], 'k 0,16': [0, 16], 'k 0,8,16': [0, 8, 16], 'k 0,8,16,24': [0, 8, 16, 24],
    'k 0..3,8..11': [0, 1, 2, 3, 8, 9, 10, 11], 'k 0,1,8,9,16,17,24,25': [0, 1, 8, 9, 16, 17, 24, 25],
}

if __name__ == '__main__':
    net = build_conv(conv_case('board3'))
    bias = np.array([(1 if j < 8 else -1) * 2.0 ** (24 + j % 8) for j in range(16)], np.float32)
    print('|out - bias| at the centre pixel; columns: bias = +2^24 .. +2^31, then -2^24 .. -2^31')
    for prec in ('bf16x3', 'f32'):
        p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=4, conv_precision=prec), 0)
        p.load_state_dict(net.state_dict())
        for name, ks in ROWS.items():
            w = np.zeros((16, 32, 3, 3), np.float32)
            w[:8, ks, 1, 1], w[8:, ks, 1, 1] = 1.0, -1.0
            out, build = p.debug_conv3x3(np.ones((1, 32, 3, 3), np.float32), w, bias)
            d = (out[0, :, 1, 1].astype(np.float64) - bias) * np.sign(bias)
            print(f'{prec:7s} {name:24s} n={len(ks):2d} ' + ' '.join('%3d' % v for v in d))
        p.close()
