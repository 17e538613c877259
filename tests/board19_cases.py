"""Board nets above 15 x 15 (tests/golden/board19_cases.npz, tools/gen_board_golden.py): the CONV_CASES format of tests/helpers.py --
name, kind, input_shape, A, blocks, planes, value_support, reward_support, seed."""

BOARD_CASES = [
    ('board19', 'board', (9, 19, 19), 362, 1, 8, 1, 1, 31),
    ('board16', 'board', (9, 16, 16), 257, 1, 8, 1, 1, 32),
]


def board_case(name):
    return next(c for c in BOARD_CASES if c[0] == name)
