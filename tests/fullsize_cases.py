"""The full-size conv nets (BASELINE.json configs C4 / C5, and C5's net on a 19 x 19 board): 128 planes x 8 residual blocks.  One table for
the reference fixtures (tests/golden/fullsize_<net>.npz, tools/gen_fullsize_golden.py), the oracle tests and the GPU tests.

FULL_CASES is in the CONV_CASES format of tests/helpers.py -- name, kind, input_shape, A, blocks, planes, value_support, reward_support,
seed; FULL[name] adds the BASELINE env count per GPU, the simulations per move and the search keywords."""

FULL_CASES = [
    ('c4', 'atari', (8, 96, 96), 6, 8, 128, 61, 61, 41),
    ('c5', 'board', (9, 15, 15), 226, 8, 128, 1, 1, 42),
    ('c5_19', 'board', (9, 19, 19), 362, 8, 128, 1, 1, 41),
]

_ATARI = dict(discount=0.997, root_dirichlet_alpha=0.25)
_BOARD = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.03)
EPS = 0.25  # root_exploration_eps of every BASELINE config

FULL = {
    # name: (case, envs per GPU, simulations per move, search keywords without root_exploration_eps)
    'c4': (FULL_CASES[0], 512, 50, _ATARI),
    'c5': (FULL_CASES[1], 256, 200, _BOARD),
    'c5_19': (FULL_CASES[2], 256, 200, _BOARD),
}
FULL19 = FULL_CASES[2]
BOARD_KW = dict(_BOARD, root_exploration_eps=EPS)

# simulations of the recorded reference search per net: the BASELINE depth for C4 and C5; C5-19 is sized to the CPU suite (the scalar
# oracle needs ~2.9 s per simulation at 19 x 19) -- its 362-wide root and the 19 x 19 conv build are the point, not the depth
FIXTURE_SIMS = {'c4': 50, 'c5': 200, 'c5_19': 20}


def full_case(name):
    return FULL[name][0]
