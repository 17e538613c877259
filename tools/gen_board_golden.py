#!/usr/bin/env python3
"""Reference fixture for board nets above 15 x 15: tests/golden/board19_cases.npz.

Runs the REFERENCE implementation (imported read-only through oracle/_refshim.py, as oracle/gen_golden.py does) on two seeded
MuZeroBoardGameNet shapes and records inputs, the random draws the reference consumed and its outputs -- never weights (the tests
rebuild them from the seed with tests/helpers.seeded_state_dict) and no reference source:
  board19  19 x 19, 362 actions (Gomoku on a Go board)
  board16  16 x 16, 257 actions (the first size past 256 actions)
each with 8 planes and 1 residual block.  Per net: two initial_inference calls with two chained recurrent_inference steps each
(2 + 4 outputs), and one uct_search (40 simulations, Dirichlet alpha 0.03, known bounds (-1, 1), board game) from a Gomoku
position a few random moves into a game.

Build container only (it needs the reference checkout):

    python tools/gen_board_golden.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))

import gen_golden as gg  # noqa: E402  (installs the reference shim)
from board19_cases import BOARD_CASES  # noqa: E402

SIMS, ALPHA = 40, 0.03


def main():
    rng = np.random.RandomState(1919)
    out = {}
    for k, case in enumerate(BOARD_CASES):
        name, ishape, A, N = case[0], case[2], case[3], case[2][1]
        net = gg.build_conv(case)
        for j in range(2):
            obs = (rng.rand(*ishape) < 0.3).astype(np.float32)
            actions = rng.randint(0, A, size=2)
            gg._infer_case(net, obs, actions, f'{name}_{j}', out)
        cfg = gg.make_config(1.0, ALPHA, SIMS, True, (-1, 1), 1, 1)
        for key, v in gg.cfg_arrays(cfg).items():
            out[f'{name}_search_{key}'] = v
        env = gg.GomokuEnv(board_size=N, stack_history=4)
        obs = env.reset()
        for _ in range(4 + 2 * k):
            legal = np.where(env.actions_mask[:N * N])[0]
            obs, _, done, _ = env.step(int(rng.choice(legal)))
            assert not done
        gg._search_case(net, cfg, obs.astype(np.float32), env.actions_mask.copy(), (env.current_player, env.opponent_player), 1.0, False,
                        1900 + k, f'{name}_search', out, A)
    path = os.path.join(REPO, 'tests', 'golden', 'board19_cases.npz')
    np.savez_compressed(path, **out)
    print(path, len(out), 'arrays')


if __name__ == '__main__':
    main()
