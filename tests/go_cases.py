"""Scripted Go games for the host and the device tests, and a numpy model of the step in the device kernel's formulation.

The boards after every ply are WRITTEN OUT BY HAND below ('.' empty, 'X' black, 'O' white, rows separated by '/'); nothing here is
printed from `games.GoEnv`.  A ply is (move, board after it[, checks]): move (r, c), 'pass' or 'resign'; checks -- `illegal` / `legal`:
points the NEXT side to move may not / may place on; `ko`: the ko point after the ply (None: none; checked where the implementation
exposes it).  A game's `end` is (the final mover's reward, the winner or None); without `end` the script stops in mid-game.

The two spirals are the exception in form only: their final positions are written out by hand, and the plies are read off them by
boards-only code (`spiral_case`: walk each colour's path from its outer end; until the last ply nothing is captured, so the board after
a ply is the board before it plus the stone).  `GoModel` is the kernel's formulation -- one propagation primitive over components of
equal cell class -- with planted mistakes (`MISTAKES`: name -> the case that must catch it)."""
import numpy as np

X, O = 1, 2


def parse(board: str) -> np.ndarray:
    rows = board.split('/')
    assert len({len(r) for r in rows}) == 1, board
    return np.array([['.XO'.index(ch) for ch in r] for r in rows], dtype=np.int8)


E5 = '...../...../...../...../.....'
E3 = '.../.../...'


def case(name, rows, cols, plies, end=None, **rules):
    return dict(name=name, rows=rows, cols=cols, plies=plies, end=end, rules=rules)


CASES = [
    # ---- captures ----
    case('capture_centre', 5, 5, [
        ((1, 2), '...../..X../...../...../.....'),
        ((2, 2), '...../..X../..O../...../.....'),
        ((2, 1), '...../..X../.XO../...../.....'),
        ('pass', '...../..X../.XO../...../.....'),
        ((2, 3), '...../..X../.XOX./...../.....'),
        ('pass', '...../..X../.XOX./...../.....'),
        ((3, 2), '...../..X../.X.X./..X../.....', dict(illegal=[(2, 2)], ko=None)),  # single-stone suicide refused; four liberties: no ko
    ]),
    case('capture_edge', 5, 5, [
        ((0, 1), '.X.../...../...../...../.....'),
        ((0, 2), '.XO../...../...../...../.....'),
        ((0, 3), '.XOX./...../...../...../.....'),
        ('pass', '.XOX./...../...../...../.....'),
        ((1, 2), '.X.X./..X../...../...../.....', dict(illegal=[(0, 2)])),
    ]),
    case('capture_corner', 5, 5, [
        ((0, 1), '.X.../...../...../...../.....'),
        ((0, 0), 'OX.../...../...../...../.....'),
        ((1, 0), '.X.../X..../...../...../.....', dict(illegal=[(0, 0)])),
    ]),
    case('capture_group', 5, 5, [
        ((1, 0), '...../X..../...../...../.....'),
        ((0, 0), 'O..../X..../...../...../.....'),
        ((1, 1), 'O..../XX.../...../...../.....'),
        ((0, 1), 'OO.../XX.../...../...../.....'),
        ((0, 2), '..X../XX.../...../...../.....', dict(ko=None)),
    ]),
    # two groups captured by one stone; before it the same point is multi-stone suicide for white and legal for black because it captures
    case('capture_two_groups', 5, 5, [
        ((0, 2), '..X../...../...../...../.....'),
        ((0, 1), '.OX../...../...../...../.....'),
        ((1, 1), '.OX../.X.../...../...../.....'),
        ((1, 0), '.OX../OX.../...../...../.....'),
        ((2, 0), '.OX../OX.../X..../...../.....', dict(illegal=[(0, 0)])),  # white there: three stones without a liberty
        ('pass', '.OX../OX.../X..../...../.....', dict(legal=[(0, 0)])),    # black there: no liberty until it captures
        ((0, 0), 'X.X../.X.../X..../...../.....', dict(ko=None, illegal=[(0, 1), (1, 0)])),  # each walled in by three black stones
    ]),
    # the capturing stone is left alone with one liberty, but it took two stones: no ko
    case('capture_two_stones_no_ko', 5, 5, [
        ((1, 1), '...../.X.../...../...../.....'),
        ((0, 1), '.O.../.X.../...../...../.....'),
        ((1, 2), '.O.../.XX../...../...../.....'),
        ((0, 2), '.OO../.XX../...../...../.....'),
        ((0, 3), '.OOX./.XX../...../...../.....'),
        ((1, 0), '.OOX./OXX../...../...../.....'),
        ((0, 0), 'X..X./OXX../...../...../.....', dict(ko=None, legal=[(0, 1), (0, 2)])),
        ((0, 1), '.O.X./OXX../...../...../.....', dict(ko=None)),  # takes the stone back at once
    ]),
    # ---- ko ----
    case('ko_retake_illegal', 5, 5, [
        ((0, 1), '.X.../...../...../...../.....'),
        ((0, 2), '.XO../...../...../...../.....'),
        ((1, 0), '.XO../X..../...../...../.....'),
        ((1, 3), '.XO../X..O./...../...../.....'),
        ((2, 1), '.XO../X..O./.X.../...../.....'),
        ((2, 2), '.XO../X..O./.XO../...../.....'),
        ((4, 4), '.XO../X..O./.XO../...../....X'),
        ((1, 1), '.XO../XO.O./.XO../...../....X'),
        ((1, 2), '.XO../X.XO./.XO../...../....X', dict(ko=(1, 1), illegal=[(1, 1)])),
    ]),
    case('ko_retake_after_ply', 5, 5, [
        ((0, 1), '.X.../...../...../...../.....'),
        ((0, 2), '.XO../...../...../...../.....'),
        ((1, 0), '.XO../X..../...../...../.....'),
        ((1, 3), '.XO../X..O./...../...../.....'),
        ((2, 1), '.XO../X..O./.X.../...../.....'),
        ((2, 2), '.XO../X..O./.XO../...../.....'),
        ((4, 4), '.XO../X..O./.XO../...../....X'),
        ((1, 1), '.XO../XO.O./.XO../...../....X'),
        ((1, 2), '.XO../X.XO./.XO../...../....X', dict(ko=(1, 1), illegal=[(1, 1)])),
        ((4, 0), '.XO../X.XO./.XO../...../O...X', dict(ko=None, legal=[(1, 1)])),
        ((3, 4), '.XO../X.XO./.XO../....X/O...X', dict(ko=None, legal=[(1, 1)])),
        ((1, 1), '.XO../XO.O./.XO../....X/O...X', dict(ko=(1, 2), illegal=[(1, 2)])),
    ]),
    case('ko_cleared_by_pass', 5, 5, [
        ((0, 1), '.X.../...../...../...../.....'),
        ((0, 2), '.XO../...../...../...../.....'),
        ((1, 0), '.XO../X..../...../...../.....'),
        ((1, 3), '.XO../X..O./...../...../.....'),
        ((2, 1), '.XO../X..O./.X.../...../.....'),
        ((2, 2), '.XO../X..O./.XO../...../.....'),
        ((4, 4), '.XO../X..O./.XO../...../....X'),
        ((1, 1), '.XO../XO.O./.XO../...../....X'),
        ((1, 2), '.XO../X.XO./.XO../...../....X', dict(ko=(1, 1), illegal=[(1, 1)])),
        ('pass', '.XO../X.XO./.XO../...../....X', dict(ko=None, legal=[(1, 1)])),  # black may fill the ko
        ((3, 4), '.XO../X.XO./.XO../....X/....X', dict(ko=None, legal=[(1, 1)])),
        ((1, 1), '.XO../XO.O./.XO../....X/....X', dict(ko=(1, 2), illegal=[(1, 2)])),
    ]),
    # ---- snapback: the capturing stone joins a group that is left with one liberty; the recapture of five stones is legal at once ----
    case('snapback', 5, 5, [
        ((1, 0), '...../X..../...../...../.....'),
        ((2, 0), '...../X..../O..../...../.....'),
        ((1, 1), '...../XX.../O..../...../.....'),
        ((2, 1), '...../XX.../OO.../...../.....'),
        ((1, 2), '...../XXX../OO.../...../.....'),
        ((2, 2), '...../XXX../OOO../...../.....'),
        ((0, 2), '..X../XXX../OOO../...../.....'),
        ((1, 3), '..X../XXXO./OOO../...../.....'),
        ('pass', '..X../XXXO./OOO../...../.....'),
        ((0, 3), '..XO./XXXO./OOO../...../.....'),
        ('pass', '..XO./XXXO./OOO../...../.....'),
        ((0, 1), '.OXO./XXXO./OOO../...../.....'),
        ((0, 0), 'X.XO./XXXO./OOO../...../.....', dict(ko=None, legal=[(0, 1)])),
        ((0, 1), '.O.O./...O./OOO../...../.....', dict(ko=None)),
    ]),
    # ---- stones at the end of one row and the start of the next share no liberty and form no group ----
    case('edge_wrap_5x5', 5, 5, [
        ((0, 4), '....X/...../...../...../.....'),
        ((0, 3), '...OX/...../...../...../.....'),
        ((1, 0), '...OX/X..../...../...../.....'),
        ((1, 4), '...O./X...O/...../...../.....'),  # (0, 4) is taken although point 5 = (1, 0) is black
        ('pass', '...O./X...O/...../...../.....'),
        ((0, 0), 'O..O./X...O/...../...../.....'),
        ('pass', 'O..O./X...O/...../...../.....'),
        ((2, 0), 'O..O./X...O/O..../...../.....'),
        ('pass', 'O..O./X...O/O..../...../.....'),
        ((1, 1), 'O..O./.O..O/O..../...../.....'),  # (1, 0) is taken although point 4 = (0, 4) is empty
    ]),
    case('edge_wrap_4x6', 4, 6, [
        ((3, 0), '....../....../....../X.....'),
        ((2, 0), '....../....../O...../X.....'),
        ((2, 5), '....../....../O....X/X.....'),
        ((3, 1), '....../....../O....X/.O....'),  # (3, 0) is taken although point 17 = (2, 5) is black and nothing lies below the last row
        ('pass', '....../....../O....X/.O....'),
        ((1, 5), '....../.....O/O....X/.O....'),
        ('pass', '....../.....O/O....X/.O....'),
        ((3, 5), '....../.....O/O....X/.O...O'),
        ('pass', '....../.....O/O....X/.O...O'),
        ((2, 4), '....../.....O/O...O./.O...O'),  # (2, 5) is taken although point 18 = (3, 0) is empty
    ]),
    # ---- ends ----
    case('end_two_passes_empty', 5, 5, [('pass', E5), ('pass', E5)], end=(1.0, O), komi2=15),  # nobody's area: the komi decides
    case('end_max_plies', 5, 5, [
        ((2, 2), '...../...../..X../...../.....'),
        ((0, 0), 'O..../...../..X../...../.....'),
        ((1, 1), 'O..../.X.../..X../...../.....'),
    ], end=(1.0, X), komi2=1, max_plies=3),  # 2 stones against 1 and half a point; the region touches both
    case('end_resign', 5, 5, [
        ((2, 2), '...../...../..X../...../.....'),
        ('resign', '...../...../..X../...../.....'),
    ], end=(-1.0, X)),
    case('end_no_resign', 5, 5, [
        ((2, 2), '...../...../..X../...../.....'),
        ('pass', '...../...../..X../...../.....'),
        ('pass', '...../...../..X../...../.....'),
    ], end=(1.0, X), allow_resign=False),  # 25 against 0 and 7.5
    # ---- counts ----
    case('count_neutral_draw', 3, 3, [
        ((0, 1), '.X./.../...'),
        ((2, 1), '.X./.../.O.'),
        ('pass', '.X./.../.O.'),
        ('pass', '.X./.../.O.'),
    ], end=(0.0, None), komi2=0),  # the one empty region touches both colours: 1 against 1
    case('count_empty_draw', 3, 3, [('pass', E3), ('pass', E3)], end=(0.0, None), komi2=0),  # a region touching nobody counts for nobody
    # seki: both groups have the same two liberties and whoever fills one is captured; the two points are neutral: 4 against 3 and half a point
    case('count_seki', 3, 3, [
        ((0, 0), 'X../.../...'),
        ((0, 2), 'X.O/.../...'),
        ((1, 0), 'X.O/X../...'),
        ((1, 2), 'X.O/X.O/...'),
        ((2, 0), 'X.O/X.O/X..'),
        ((2, 2), 'X.O/X.O/X.O'),
        ((1, 1), 'X.O/XXO/X.O', dict(legal=[(0, 1), (2, 1)])),
        ('pass', 'X.O/XXO/X.O', dict(legal=[(0, 1), (2, 1)])),
        ('pass', 'X.O/XXO/X.O'),
    ], end=(1.0, X), komi2=1),
    case('count_seki_draw', 3, 3, [
        ((0, 0), 'X../.../...'),
        ((0, 2), 'X.O/.../...'),
        ((1, 0), 'X.O/X../...'),
        ((1, 2), 'X.O/X.O/...'),
        ((2, 0), 'X.O/X.O/X..'),
        ((2, 2), 'X.O/X.O/X.O'),
        ((1, 1), 'X.O/XXO/X.O'),
        ('pass', 'X.O/XXO/X.O'),
        ('pass', 'X.O/XXO/X.O'),
    ], end=(0.0, None), komi2=2),
    case('final_pass_loses', 5, 5, [
        ('pass', E5),
        ((1, 1), '...../.O.../...../...../.....'),
        ((3, 3), '...../.O.../...../...X./.....'),
        ('pass', '...../.O.../...../...X./.....'),  # (the pass before the last was black's first ply: a placement lies between)
        ('pass', '...../.O.../...../...X./.....'),
    ], end=(-1.0, O), komi2=15),
]

# ---- the long group: one spiral of black stones with a single liberty, taken by one white stone ----
SPIRAL_9 = [
    'XXXXXXXXX',
    'OOOOOOOOX',
    'XXXXXXXOX',
    'XOOOOOXOX',
    'XOXXXOXOX',
    'XOX.OOXOX',
    'XOXXXXXOX',
    'XOOOOOOOX',
    'XXXXXXXXX',
]
SPIRAL_19 = [
    'XXXXXXXXXXXXXXXXXXX',
    'OOOOOOOOOOOOOOOOOOX',
    'XXXXXXXXXXXXXXXXXOX',
    'XOOOOOOOOOOOOOOOXOX',
    'XOXXXXXXXXXXXXXOXOX',
    'XOXOOOOOOOOOOOXOXOX',
    'XOXOXXXXXXXXXOXOXOX',
    'XOXOXOOOOOOOXOXOXOX',
    'XOXOXOXXXXXOXOXOXOX',
    'XOXOXOXOO.XOXOXOXOX',
    'XOXOXOXOXXXOXOXOXOX',
    'XOXOXOXOOOOOXOXOXOX',
    'XOXOXOXXXXXXXOXOXOX',
    'XOXOXOOOOOOOOOXOXOX',
    'XOXOXXXXXXXXXXXOXOX',
    'XOXOOOOOOOOOOOOOXOX',
    'XOXXXXXXXXXXXXXXXOX',
    'XOOOOOOOOOOOOOOOOOX',
    'XXXXXXXXXXXXXXXXXXX',
]


def _walk(grid: np.ndarray, start, colour):
    """The stones of `colour` in path order from `start` (boards-only: every stone of a spiral arm has at most two neighbours of its colour)."""
    rows, cols = grid.shape
    path, seen = [start], {start}
    while True:
        r, c = path[-1]
        nxt = [q for q in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1))
               if 0 <= q[0] < rows and 0 <= q[1] < cols and grid[q] == colour and q not in seen]
        if not nxt:
            return path
        assert len(nxt) == 1, (path[-1], nxt)
        path.append(nxt[0])
        seen.add(nxt[0])


def board_str(grid: np.ndarray) -> str:
    return '/'.join(''.join('.XO'[v] for v in row) for row in grid)


def spiral_case(name, pattern):
    """Black and white lay their arms from the outside in, black first; white passes once its arm is done, then takes black's last
    liberty.  Nothing is captured before that ply, so every earlier board is the one before it plus the stone."""
    final = parse('/'.join(pattern))
    n = final.shape[0]
    black, white = _walk(final, (0, 0), X), _walk(final, (1, 0), O)
    assert len(black) == np.count_nonzero(final == X) and len(white) == np.count_nonzero(final == O) and len(black) > len(white)
    (hole,) = [tuple(q) for q in np.argwhere(final == 0)]
    grid = np.zeros_like(final)
    plies = []
    for i, stone in enumerate(black):
        grid[stone] = X
        plies.append((stone, board_str(grid)))
        if i < len(white):
            grid[white[i]] = O
            plies.append((white[i], board_str(grid)))
        elif i < len(black) - 1:
            plies.append(('pass', board_str(grid)))
    assert np.array_equal(grid, final)
    grid[grid == X] = 0  # the whole arm comes off
    grid[hole] = O
    plies.append((hole, board_str(grid), dict(ko=None)))
    return case(name, n, n, plies)


SPIRAL_CASES = [spiral_case('spiral_9x9', SPIRAL_9), spiral_case('spiral_19x19', SPIRAL_19)]


def sparse(rows, cols, black=(), white=()):
    """A large board written as its stones."""
    grid = np.zeros((rows, cols), np.int8)
    for p in black:
        grid[p] = X
    for p in white:
        grid[p] = O
    return board_str(grid)


# 19 x 19 by hand: a capture in the far corner (points 341, 359, 360: past 256), then a ko on the last two rows
BIG_CASES = [
    case('far_corner_19x19', 19, 19, [
        ((18, 17), sparse(19, 19, [(18, 17)])),
        ((18, 18), sparse(19, 19, [(18, 17)], [(18, 18)])),
        ((17, 18), sparse(19, 19, [(18, 17), (17, 18)]), dict(illegal=[(18, 18)], ko=None)),
        ((17, 17), sparse(19, 19, [(18, 17), (17, 18)], [(17, 17)])),
        ('pass', sparse(19, 19, [(18, 17), (17, 18)], [(17, 17)])),
        ((18, 16), sparse(19, 19, [(18, 17), (17, 18)], [(17, 17), (18, 16)])),
        ('pass', sparse(19, 19, [(18, 17), (17, 18)], [(17, 17), (18, 16)])),
        ((18, 18), sparse(19, 19, [(17, 18)], [(17, 17), (18, 16), (18, 18)]), dict(ko=(18, 17), illegal=[(18, 17)])),  # point 359
    ]),
]
ALL_CASES = CASES + SPIRAL_CASES + BIG_CASES
DEFAULT_RULES = dict(komi2=15, max_plies=0, allow_resign=True)


def rules_of(c) -> dict:
    return dict(DEFAULT_RULES, **c['rules'])


def groups():
    """The cases by (rows, cols, rules): what one device planner can play side by side."""
    out = {}
    for c in ALL_CASES:
        out.setdefault((c['rows'], c['cols']) + tuple(sorted(rules_of(c).items())), []).append(c)
    return out
BY_NAME = {c['name']: c for c in ALL_CASES}


def action_of(c, move) -> int:
    nn = c['rows'] * c['cols']
    return nn if move == 'pass' else nn + 1 if move == 'resign' else move[0] * c['cols'] + move[1]


# ---------------------------------------------------------------------------------------------------------
# the numpy model: GoEnv.step in the device kernel's formulation
# ---------------------------------------------------------------------------------------------------------
NONE_LO, NONE_HI = 0x7fff, -1

# planted mistake -> the scripted game that must catch it
MISTAKES = {
    'suicide_before_captures': 'capture_two_groups',   # the suicide test made before the captures are taken off
    'ko_survives_pass': 'ko_cleared_by_pass',
    'ko_on_two_stones': 'capture_two_stones_no_ko',
    'ko_when_joining_group': 'snapback',
    'wrap_right': 'edge_wrap_5x5',                     # the right neighbour of a row's last point: the next row's first
    'wrap_left': 'edge_wrap_5x5',
    'wrap_up': 'capture_edge',                         # above the first row: the last row
    'wrap_down': 'edge_wrap_4x6',                      # below the last row: the first row
    'rounds_capped': 'spiral_9x9',                     # the propagation stops after 8 rounds
    'neutral_awarded': 'count_neutral_draw',           # a region touching both colours counts for black
    'komi_to_black': 'end_two_passes_empty',
    'pass_flag_survives_placement': 'final_pass_loses',
    'max_plies_off_by_one': 'end_max_plies',
    'opponent_history_stale': 'capture_centre',        # the opponent's history is not advanced on a capture
}


class GoModel:
    """`games.GoEnv`'s interface (board, actions_mask, current_player, steps, winner, step, observation) computed as mz_go.h computes
    it: cell classes, neighbour tables, and ONE primitive -- (lo, hi) of every cell becomes (min, max) over its 4-connected component
    of equal class, Jacobi rounds bounded by nn."""

    def __init__(self, rows=9, cols=9, komi2=15, max_plies=0, allow_resign=True, stack_history=4, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.rows, self.cols, self.nn = rows, cols, rows * cols
        self.komi2, self.max_plies, self.allow_resign = komi2, max_plies or 2 * rows * cols, allow_resign
        self.stack_history, self.mistake = stack_history, mistake
        self.num_actions = self.nn + 2
        nn, idx = self.nn, np.arange(rows * cols)
        r, c = idx // cols, idx % cols
        up = np.where(r > 0, idx - cols, -1)
        down = np.where(r < rows - 1, idx + cols, -1)
        left = np.where(c > 0, idx - 1, -1)
        right = np.where(c < cols - 1, idx + 1, -1)
        if mistake == 'wrap_up':
            up = (idx - cols) % nn
        if mistake == 'wrap_down':
            down = (idx + cols) % nn
        if mistake == 'wrap_left':
            left = np.where(idx > 0, idx - 1, -1)
        if mistake == 'wrap_right':
            right = np.where(idx < nn - 1, idx + 1, -1)
        self.nb = np.stack([up, down, left, right])  # [4, nn], -1: off the board
        self.reset()

    def reset(self):
        self.cells = np.zeros(self.nn, np.int8)
        self.current_player, self.steps, self.winner, self.finished = 1, 0, None, False
        self.ko, self.passf = -1, False
        self.planes = np.zeros((2, self.stack_history, self.nn), np.int8)
        self.actions_mask = np.ones(self.num_actions, np.bool_)
        self.actions_mask[self.nn + 1] = self.allow_resign
        return self.observation()

    @property
    def board(self):
        return self.cells.reshape(self.rows, self.cols)

    @property
    def is_game_over(self):
        return self.winner is not None or self.finished

    def _nb_cls(self, cells):
        return np.where(self.nb >= 0, cells[np.maximum(self.nb, 0)], 3)  # [4, nn] the neighbours' classes (3: off the board)

    def propagate(self, cells, lo, hi):
        same = self._nb_cls(cells) == cells[None, :]
        q = np.maximum(self.nb, 0)
        rounds = 8 if self.mistake == 'rounds_capped' else self.nn
        for _ in range(rounds):
            l = np.minimum(lo, np.where(same, lo[q], NONE_LO).min(axis=0))
            h = np.maximum(hi, np.where(same, hi[q], NONE_HI).max(axis=0))
            if np.array_equal(l, lo) and np.array_equal(h, hi):
                break
            lo, hi = l, h
        return lo, hi

    def liberties(self, cells):
        """(lo, hi) per cell: the smallest and the largest liberty of the stone's group (NONE_LO / NONE_HI: none)."""
        empty_nb = self._nb_cls(cells) == 0
        stone = (cells == 1) | (cells == 2)
        lo = np.where(stone, np.where(empty_nb, self.nb, NONE_LO).min(axis=0), NONE_LO)
        hi = np.where(stone, np.where(empty_nb, self.nb, NONE_HI).max(axis=0), NONE_HI)
        return self.propagate(cells, lo, hi)

    def all_groups_have_liberty(self, cells) -> bool:
        cells = np.asarray(cells, np.int8).reshape(-1)
        _, hi = self.liberties(cells)
        return bool(np.all(hi[cells != 0] >= 0))

    def areas(self, cells):
        ncls = self._nb_cls(cells)
        tb, tw = (ncls == 1).any(axis=0), (ncls == 2).any(axis=0)
        lo = np.where((cells == 0) & tb, 0, 1)
        hi = np.where((cells == 0) & tw, 1, 0)
        lo, hi = self.propagate(cells, lo, hi)
        black = (cells == 1) | ((cells == 0) & (lo == 0) & (hi == 0))
        white = (cells == 2) | ((cells == 0) & (lo == 1) & (hi == 1))
        if self.mistake == 'neutral_awarded':
            black = black | ((cells == 0) & (lo == 0) & (hi == 1))
        return int(black.sum()), int(white.sum())

    def legal_mask(self, cells, nxt, ko):
        """The placements of colour `nxt` on `cells` (every group of which has a liberty)."""
        lo, hi = self.liberties(cells)
        q = np.maximum(self.nb, 0)
        ncls = self._nb_cls(cells)
        one = (lo == hi)[q]  # the neighbour's group has exactly one liberty: this point
        captures = (ncls == 3 - nxt) & one
        if self.mistake == 'suicide_before_captures':  # the stone is judged before the stones it takes come off
            captures[:] = False
        ok = (ncls == 0) | ((ncls == nxt) & ~one) | captures
        legal = (cells == 0) & ok.any(axis=0)
        if ko >= 0:
            legal[ko] = False
        return legal

    def step(self, action):
        assert not self.is_game_over and self.actions_mask[action], action
        nn, me, opp = self.nn, self.current_player, 3 - self.current_player
        placed, passed, resign = action < nn, action == nn, action > nn
        cells, reward, ko = self.cells.copy(), 0.0, -1
        limit = self.max_plies + (1 if self.mistake == 'max_plies_off_by_one' else 0)
        done = resign or (passed and self.passf) or self.steps + 1 == limit
        captured_any = False
        if placed:
            cells[action] = me
            lo, hi = self.liberties(cells)
            captured = (cells == opp) & (hi < 0)
            cells[captured] = 0
            captured_any = bool(captured.any())
            ncap = int(captured.sum())
            ncls = self._nb_cls(cells)[:, action]
            own, empty = int((ncls == me).sum()), int((ncls == 0).sum())
            single = own == 0 or self.mistake == 'ko_when_joining_group'
            if (ncap == 1 or (self.mistake == 'ko_on_two_stones' and ncap == 2)) and single and empty == 1:
                ko = int(np.flatnonzero(captured)[0])
        elif passed and self.mistake == 'ko_survives_pass':
            ko = self.ko
        if resign:
            reward, self.winner = -1.0, opp
        else:
            self.cells = cells
            for p in (1, 2):
                if p == opp and captured_any and self.mistake == 'opponent_history_stale':
                    continue
                self.planes[p - 1, 1:] = self.planes[p - 1, :-1].copy()
                self.planes[p - 1, 0] = cells == p
            if done:
                black, white = self.areas(cells)
                diff = 2 * black - 2 * white + (self.komi2 if self.mistake == 'komi_to_black' else -self.komi2)
                self.finished = True
                if diff != 0:
                    self.winner = 1 if diff > 0 else 2
                    reward = 1.0 if self.winner == me else -1.0
            self.ko = ko
            self.passf = passed or (self.passf and self.mistake == 'pass_flag_survives_placement')
        if not done:
            self.current_player = opp
            self.actions_mask[:nn] = self.legal_mask(cells, opp, ko)
        self.steps += 1
        return self.observation(), reward, done, {}

    def observation(self):
        me = self.current_player - 1
        out = np.zeros((2 * self.stack_history + 1, self.rows, self.cols), np.int8)
        out[0:2 * self.stack_history:2] = self.planes[me].reshape(-1, self.rows, self.cols)
        out[1:2 * self.stack_history:2] = self.planes[1 - me].reshape(-1, self.rows, self.cols)
        out[-1] = 1 if me == 0 else 0
        return out


# ---------------------------------------------------------------------------------------------------------
# running a scripted game on anything with GoEnv's interface
# ---------------------------------------------------------------------------------------------------------
def expected_observation(c, boards, n_plies, to_move, stack_history):
    """The observation after `n_plies` plies from the hand-written boards alone: plane k of a colour is its stones k plies ago (a
    fresh game: nothing)."""
    out = np.zeros((2 * stack_history + 1, c['rows'], c['cols']), np.int8)
    for k in range(stack_history):
        if n_plies - k >= 1:
            b = boards[n_plies - k - 1]
            out[2 * k] = b == to_move
            out[2 * k + 1] = b == 3 - to_move
    out[-1] = 1 if to_move == 1 else 0
    return out


def run_case(c, env, ko_of=None):
    """Plays `c` on `env` and checks every ply against the hand-written boards.  Raises AssertionError naming the case and the ply."""
    nn, cols = c['rows'] * c['cols'], c['cols']
    allow = c['rules'].get('allow_resign', True)
    boards = [parse(p[1]) for p in c['plies']]
    assert not env.board.any() and env.actions_mask[:nn + 1].all() and bool(env.actions_mask[nn + 1]) == allow, c['name']
    for i, ply in enumerate(c['plies']):
        where = f"{c['name']} ply {i + 1}"
        a = action_of(c, ply[0])
        mover = 1 + i % 2
        assert env.current_player == mover, where
        assert env.actions_mask[a], f'{where}: the scripted move is not legal'
        obs, reward, done, _ = env.step(a)
        assert np.array_equal(env.board, boards[i]), f'{where}: board\n{board_str(env.board)}\nexpected\n{ply[1]}'
        last = i == len(c['plies']) - 1
        if last and c['end'] is not None:
            assert done and reward == c['end'][0] and env.winner == c['end'][1], f'{where}: end {done} {reward} {env.winner}'
            continue
        assert not done and reward == 0.0, f'{where}: unexpected end'
        assert env.current_player == 3 - mover and env.steps == i + 1, where
        sh = (obs.shape[0] - 1) // 2
        assert np.array_equal(obs, expected_observation(c, boards, i + 1, 3 - mover, sh)), f'{where}: observation'
        m = env.actions_mask
        assert m[nn] and bool(m[nn + 1]) == allow, f'{where}: pass / resign entries'
        assert not m[:nn][boards[i].reshape(-1) != 0].any(), f'{where}: an occupied point is legal'
        checks = ply[2] if len(ply) > 2 else {}
        for (r, cc) in checks.get('illegal', []):
            assert not m[r * cols + cc], f'{where}: ({r}, {cc}) must be illegal'
        for (r, cc) in checks.get('legal', []):
            assert m[r * cols + cc], f'{where}: ({r}, {cc}) must be legal'
        if 'ko' in checks and ko_of is not None:
            want = None if checks['ko'] is None else checks['ko'][0] * cols + checks['ko'][1]
            assert ko_of(env) == want, f'{where}: ko point {ko_of(env)}, expected {want}'
