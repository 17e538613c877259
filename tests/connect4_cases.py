"""Scripted Connect Four games with hand-written expected boards, and a numpy model of the device step (csrc/mz_connect4.h).

Shapes, the smallest at which each thing can still go wrong:
  S  4 rows x 5 cols, 3 to win: 20 points (more than a 16-lane group), both diagonals fit;
  T  5 x 4, 4 to win: more rows than columns, a horizontal win spans the full width;
  F  6 x 7, 4 to win: the game itself.
A case: `moves` (column per ply, black first; the column count resigns), `board` the position after the last move (rows top to bottom,
'.' empty, 'X' black, 'O' white), `reward` / `done` of the last move and `winner` (1 black, 2 white, None).  Every earlier move has
reward 0 and done False.  `masks` (where given): the legal columns after every ply.  The short games were composed by hand; the move
lists of the long ones (draws, wins on the last cell, T's and F's diagonals and long lines) were found by random play and their boards
written down from the position reached, then read through; tests/test_connect4_host.py checks what each case claims about itself.

`C4Model` is the kernel's formulation in numpy: one byte per point, the two colours' bitboards (bit = row * cols + column) rebuilt from
the bytes, gravity from the popcount of the occupancy under the column mask, the win test by walking the eight rays from the placed stone
with explicit row and column bounds, the history shift, the next side's observation, the mask, the auto-reset.  `bug` plants one mistake."""
import numpy as np

SHAPES = {'S': (4, 5, 3), 'T': (5, 4, 4), 'F': (6, 7, 4)}


def _case(name, shape, moves, board, reward=0.0, done=False, winner=None, masks=None):
    return dict(name=name, shape=shape, moves=moves, board=board, reward=reward, done=done, winner=winner, masks=masks)


CASES = [
    # ---- S: 4 x 5, 3 to win; the win test opens at ply 4 ----
    _case('vertical_earliest_win', 'S', [0, 1, 0, 1, 0], ['.....', 'X....', 'XO...', 'XO...'], 1.0, True, 1),
    _case('horizontal_left', 'S', [0, 0, 1, 1, 2], ['.....', '.....', 'OO...', 'XXX..'], 1.0, True, 1),
    _case('horizontal_middle', 'S', [1, 1, 2, 2, 3], ['.....', '.....', '.OO..', '.XXX.'], 1.0, True, 1),
    _case('horizontal_right', 'S', [2, 2, 3, 3, 4], ['.....', '.....', '..OO.', '..XXX'], 1.0, True, 1),
    _case('diag_up_last_top', 'S', [0, 1, 1, 2, 4, 2, 2], ['.....', '..X..', '.XO..', 'XOO.X'], 1.0, True, 1),
    _case('diag_up_last_bottom', 'S', [1, 2, 1, 2, 2, 4, 0], ['.....', '..X..', '.XO..', 'XXO.O'], 1.0, True, 1),
    _case('diag_down_last_top', 'S', [4, 3, 3, 2, 0, 2, 2], ['.....', '..X..', '..OX.', 'X.OOX'], 1.0, True, 1),
    _case('diag_down_last_bottom', 'S', [3, 2, 3, 2, 2, 0, 4], ['.....', '..X..', '..OX.', 'O.OXX'], 1.0, True, 1),
    _case('long_line_middle', 'S', [0, 0, 1, 1, 3, 3, 2], ['.....', '.....', 'OO.O.', 'XXXX.'], 1.0, True, 1),  # four in a row, the third stone last
    _case('both_rays_needed', 'S', [4, 1, 2, 4, 3], ['.....', '.....', '....O', '.OXXX'], 1.0, True, 1),  # X . X, then the middle
    # num_to_win stones at consecutive bit positions across a row edge: NOT a line
    _case('wrap_horizontal', 'S', [0, 3, 3, 4, 4], ['.....', '.....', '...XX', 'X..OO']),  # bits 13, 14, 15
    _case('wrap_diag_up', 'S', [3, 0, 0, 4, 4], ['.....', '.....', 'X...X', 'O..XO']),  # bits 18, 14, 10: (3,3) (2,4) | (2,0)
    _case('wrap_diag_down', 'S', [1, 4, 4, 4, 4, 0, 0], ['....X', '....O', 'X...X', 'OX..O']),  # bits 4, 10, 16: (0,4) | (2,0) (3,1)
    _case('column_fills', 'S', [2, 2, 2, 2], ['..O..', '..X..', '..O..', '..X..'],
          masks=[[0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 1, 3, 4]]),
    _case('draw_full_board', 'S', [1, 3, 3, 3, 0, 1, 4, 0, 0, 0, 1, 2, 3, 4, 2, 2, 2, 1, 4, 4], ['OOXXO', 'XXOOX', 'OOXXO', 'XXOOX'], 0.0, True, None),
    _case('win_on_last_cell', 'S', [0, 0, 0, 3, 4, 4, 4, 2, 1, 0, 3, 4, 2, 2, 2, 1, 1, 3, 1, 3], ['OXXOO', 'XXOOX', 'OOXXO', 'XXOOX'], 1.0, True, 2),
    _case('resign_black', 'S', [5], ['.....', '.....', '.....', '.....'], -1.0, True, 2),
    _case('resign_white', 'S', [0, 5], ['.....', '.....', '.....', 'X....'], -1.0, True, 1),
    # ---- T: 5 x 4, 4 to win; the win test opens at ply 6; a horizontal line touches both edges ----
    _case('vertical_earliest_win', 'T', [0, 1, 0, 1, 0, 1, 0], ['....', 'X...', 'XO..', 'XO..', 'XO..'], 1.0, True, 1),
    _case('horizontal_full_width', 'T', [0, 0, 1, 1, 2, 2, 3], ['....', '....', '....', 'OOO.', 'XXXX'], 1.0, True, 1),
    _case('both_rays_needed', 'T', [0, 0, 1, 1, 3, 3, 2], ['....', '....', '....', 'OO.O', 'XXXX'], 1.0, True, 1),
    _case('diag_up_last_top', 'T', [0, 1, 1, 2, 2, 3, 2, 3, 3, 0, 3], ['....', '...X', '..XX', 'OXXO', 'XOOO'], 1.0, True, 1),
    _case('diag_up_last_bottom', 'T', [2, 2, 2, 3, 1, 2, 3, 3, 3, 3, 1, 2, 0], ['..OO', '..OX', '..XO', '.XOX', 'XXXO'], 1.0, True, 1),
    _case('diag_down_last_top', 'T', [3, 1, 2, 3, 2, 1, 0, 0, 1, 0, 0], ['....', 'X...', 'OX..', 'OOXO', 'XOXX'], 1.0, True, 1),
    _case('diag_down_last_bottom', 'T', [1, 1, 2, 0, 0, 1, 1, 2, 0, 0, 0, 3], ['X...', 'OX..', 'XO..', 'XOO.', 'OXXO'], 1.0, True, 2),
    _case('wrap_horizontal', 'T', [0, 1, 1, 2, 2, 3, 3], ['....', '....', '....', '.XXX', 'XOOO']),  # bits 13, 14, 15, 16
    _case('wrap_diag_up', 'T', [2, 3, 1, 1, 1, 0, 0, 2, 3], ['....', '....', '.X..', 'XOOX', 'OXXO']),  # bits 18, 15, 12, 9
    _case('wrap_diag_down', 'T', [0, 0, 2, 1, 2, 2, 2, 2, 3, 3, 3, 3], ['..O.', '..XO', '..OX', 'O.XO', 'XOXX']),  # bits 2, 7, 12, 17 (white)
    _case('column_fills', 'T', [1, 1, 1, 1, 1], ['.X..', '.O..', '.X..', '.O..', '.X..'],
          masks=[[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [0, 2, 3]]),
    _case('draw_full_board', 'T', [1, 2, 3, 3, 2, 0, 1, 1, 1, 1, 0, 2, 0, 0, 2, 3, 0, 2, 3, 3], ['XOOO', 'OXXX', 'XOOO', 'XXXO', 'OXOX'], 0.0, True, None),
    _case('win_on_last_cell', 'T', [2, 3, 0, 3, 2, 3, 3, 1, 1, 1, 0, 1, 1, 2, 0, 2, 3, 0, 2, 0], ['OXXX', 'OOOX', 'XOOO', 'XXXO', 'XOXO'], 1.0, True, 2),
    _case('resign_black', 'T', [4], ['....', '....', '....', '....', '....'], -1.0, True, 2),
    _case('resign_white', 'T', [0, 4], ['....', '....', '....', '....', 'X...'], -1.0, True, 1),
    # ---- F: 6 x 7, 4 to win; the win test opens at ply 6 ----
    _case('vertical_earliest_win', 'F', [0, 1, 0, 1, 0, 1, 0], ['.......', '.......', 'X......', 'XO.....', 'XO.....', 'XO.....'], 1.0, True, 1),
    _case('horizontal_left', 'F', [2, 5, 0, 5, 1, 0, 2, 2, 3], ['.......', '.......', '.......', '..O....', 'O.X..O.', 'XXXX.O.'], 1.0, True, 1),
    _case('horizontal_middle', 'F', [1, 5, 4, 5, 2, 5, 5, 4, 4, 5, 5, 2, 3], ['.....X.', '.....O.', '.....X.', '....XO.', '..O.OO.', '.XXXXO.'], 1.0, True, 1),
    _case('horizontal_right', 'F', [3, 0, 3, 0, 4, 2, 5, 3, 6], ['.......', '.......', '.......', '...O...', 'O..X...', 'O.OXXXX'], 1.0, True, 1),
    _case('both_rays_needed', 'F', [3, 0, 3, 0, 4, 2, 6, 3, 5], ['.......', '.......', '.......', '...O...', 'O..X...', 'O.OXXXX'], 1.0, True, 1),
    _case('diag_up_last_top', 'F', [4, 4, 0, 3, 3, 6, 4, 5, 5, 6, 2, 5, 5], ['.......', '.......', '.....X.', '....XO.', '...XOXO', 'X.XOXOO'], 1.0, True, 1),
    _case('diag_up_last_bottom', 'F', [6, 3, 5, 5, 5, 4, 4, 5, 0, 3, 6, 4, 5, 2], ['.......', '.....X.', '.....O.', '....OX.', '...OXOX', 'X.OOOXX'], 1.0, True, 2),
    _case('diag_down_last_top', 'F', [3, 6, 2, 1, 4, 2, 1, 1, 2, 0, 3, 3, 1], ['.......', '.......', '.X.....', '.OXO...', '.XOX...', 'OOXXX.O'], 1.0, True, 1),
    _case('diag_down_last_bottom', 'F', [1, 2, 1, 2, 0, 2, 0, 4, 0, 1, 2, 0, 2, 3], ['.......', '..X....', 'O.X....', 'XOO....', 'XXO....', 'XXOOO..'], 1.0, True, 2),
    _case('long_line_middle', 'F', [6, 1, 1, 6, 5, 1, 4, 5, 6, 5, 2, 2, 3], ['.......', '.......', '.......', '.O...OX', '.XO..OO', '.OXXXXX'], 1.0, True, 1),
    _case('wrap_horizontal', 'F', [0, 4, 4, 5, 5, 6, 6], ['.......', '.......', '.......', '.......', '....XXX', 'X...OOO']),  # bits 32 .. 35
    _case('wrap_diag_up', 'F', [5, 6, 1, 1, 1, 0, 0, 3, 6], ['.......', '.......', '.......', '.X.....', 'XO....X', 'OX.O.XO']),  # bits 40, 34, 28, 22
    _case('wrap_diag_down', 'F', [0, 0, 5, 1, 5, 5, 5, 5, 6, 6, 6, 6], ['.......', '.....O.', '.....XO', '.....OX', 'O....XO', 'XO...XX']),  # bits 12, 20, 28, 36 (white)
    _case('column_fills', 'F', [3, 3, 3, 3, 3, 3], ['...O...', '...X...', '...O...', '...X...', '...O...', '...X...'],
          masks=[[0, 1, 2, 3, 4, 5, 6]] * 5 + [[0, 1, 2, 4, 5, 6]]),
    _case('draw_full_board', 'F', [4, 6, 5, 1, 5, 3, 0, 0, 0, 5, 5, 6, 1, 0, 4, 1, 6, 5, 5, 3, 1, 0, 0, 6, 4, 4, 2, 1, 1, 6, 3, 4, 2, 4, 6, 3, 3, 3, 2, 2, 2, 2],
          ['XXOOOXX', 'OOXXOOO', 'OXOOOXO', 'XOXXXOX', 'OXXOXXO', 'XOXOXXO'], 0.0, True, None),
    _case('win_on_last_cell', 'F', [3, 6, 2, 1, 2, 2, 3, 6, 1, 5, 2, 2, 0, 2, 5, 5, 6, 4, 3, 1, 6, 0, 6, 6, 0, 4, 4, 3, 4, 0, 0, 5, 4, 4, 1, 1, 0, 5, 1, 3, 3, 5],
          ['XXOXOOO', 'XOOOXOX', 'OXXOXOX', 'XOOXXOX', 'OXXXOXO', 'XOXXOOO'], 1.0, True, 2),
    _case('resign_black', 'F', [7], ['.......'] * 6, -1.0, True, 2),
    _case('resign_white', 'F', [0, 7], ['.......'] * 5 + ['X......'], -1.0, True, 1),
]


def cases(shape):
    return [c for c in CASES if c['shape'] == shape]


def case(shape, name):
    return next(c for c in CASES if c['shape'] == shape and c['name'] == name)


def board_array(rows_text):
    return np.array([['.XO'.index(ch) for ch in row] for row in rows_text], np.int8)


def observation_from_boards(boards_after_own_moves, to_play, stack_history, rows, cols):
    """BoardGameEnv's observation written from board snapshots, not from shifted planes: `boards_after_own_moves[p]` lists the boards as
    they stood after each of player p's moves, newest first.  Plane 2k: the stones of the side to move after its k-th newest move; plane
    2k + 1: the opponent's likewise; the last plane: 1 where black is to move."""
    out = np.zeros((2 * stack_history + 1, rows, cols), np.int8)
    for k in range(stack_history):
        for j, p in enumerate((to_play, 3 - to_play)):
            snaps = boards_after_own_moves[p]
            if k < len(snaps):
                out[2 * k + j] = snaps[k] == p
    out[-1] = 1 if to_play == 1 else 0
    return out


BUGS = ('no_guard', 'gravity_high', 'diag_missing', 'one_ray', 'mask_early', 'mask_late', 'draw_first', 'switch_after_end', 'wrong_history',
        'gate_off_by_one', 'resign_wrong_side')


class C4Model:
    """The device step of one env, in the kernel's formulation (see the module docstring)."""

    def __init__(self, rows, cols, win, bug=None):
        assert bug is None or bug in BUGS
        self.rows, self.cols, self.win, self.bug = rows, cols, win, bug
        self.nn, self.A = rows * cols, cols + 1
        self.episodes = 0
        self._fresh()

    def _fresh(self):
        self.board = np.zeros(self.nn, np.int8)
        self.planes = np.zeros((2, 4, self.nn), np.int8)
        self.mask = np.ones(self.A, np.uint8)
        self.player, self.steps = 1, 0
        self.obs = np.zeros((9, self.nn), np.float32)
        self.obs[8] = 1.0

    def _ray(self, stones, r, c, dr, dc):
        k = 0
        r, c = r + dr, c + dc
        while 0 <= r < self.rows and (self.bug == 'no_guard' or 0 <= c < self.cols):
            p = r * self.cols + c
            if not (0 <= p < self.nn and (stones >> p) & 1):
                break
            k, r, c = k + 1, r + dr, c + dc
        return k

    def step(self, a):
        """Returns dict(reward, done, winner, board: the position after the move and before any reset, to_play: the side to move
        after the move and before any reset)."""
        rows, cols, nn = self.rows, self.cols, self.nn
        me, opp, st = self.player, 3 - self.player, self.steps
        black = sum(1 << int(i) for i in np.flatnonzero(self.board == 1))
        white = sum(1 << int(i) for i in np.flatnonzero(self.board == 2))
        occ, full = black | white, (1 << nn) - 1
        mine = black if me == 1 else white
        winner, reward, p, row = 0, 0.0, -1, -1
        if a >= cols:
            reward = -1.0
            winner = me if self.bug == 'resign_wrong_side' else opp
        else:
            colmask = sum(1 << (r * cols + a) for r in range(rows))
            height = bin(occ & colmask).count('1')
            row = rows - 1 - height - (1 if self.bug == 'gravity_high' and height < rows - 1 else 0)
            p = row * cols + a
            mine |= 1 << p
            gate = (self.win - 1) * 2 + (1 if self.bug == 'gate_off_by_one' else 0)
            if st >= gate:
                dirs = [(0, 1), (1, 0), (1, 1), (-1, 1)]
                if self.bug == 'diag_missing':
                    dirs = dirs[:3]
                for dr, dc in dirs:
                    n = 1 + self._ray(mine, row, a, dr, dc) + (0 if self.bug == 'one_ray' else self._ray(mine, row, a, -dr, -dc))
                    if n >= self.win:
                        winner = me
                if winner:
                    reward = 1.0
        is_full = p >= 0 and (occ | (1 << p)) == full
        if self.bug == 'draw_first' and is_full:
            winner, reward = 0, 0.0
        done = winner != 0 or is_full
        after = self.board.copy()
        if p >= 0:
            after[p] = me
        out = dict(reward=reward, done=done, winner=winner or None, board=after.reshape(rows, cols),
                   to_play=me if done and self.bug != 'switch_after_end' else opp)
        if not done:
            shifted = (opp if self.bug == 'wrong_history' else me) - 1
            hist = self.planes[shifted]
            hist[1:] = hist[:-1].copy()
            hist[0] = (np.uint64(mine) >> np.arange(nn, dtype=np.uint64)) & np.uint64(1)
            self.board = after
            clear_at = {'mask_early': 1, 'mask_late': -1}.get(self.bug, 0)
            if row == clear_at:
                self.mask[a] = 0
            self.player, self.steps = opp, st + 1
            self.obs[0:8:2] = self.planes[opp - 1]
            self.obs[1:8:2] = self.planes[me - 1]
            self.obs[8] = 1.0 if opp == 1 else 0.0
        else:
            self.episodes += 1
            self._fresh()
        return out
