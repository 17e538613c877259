"""Host-side environments: `BoardGameEnv` semantics of the reference (`games/env.py:40-365`) with the win test of
`games/tictactoe.py:33-77` / `games/gomoku.py:72-116` (n in a row through the last move only), and the observation wrappers of
`gym_env.py`.  The device-resident self-play has its own copies of the board games and CartPole (`csrc/mz_env.h`, same rules);
these classes serve evaluators, tools and host-stepped self-play (`pipeline.run_self_play` with env objects)."""
from typing import Optional, Tuple

import numpy as np


class BoardGameEnv:
    """N x N board, players 1 (black, moves first) and 2 (white); action N*N resigns (`enable_resign`)."""

    def __init__(self, board_size: int = 15, stack_history: int = 4, num_to_win: int = 5, black_player_id: int = 1, white_player_id: int = 2,
                 enable_resign: bool = True, name: str = '') -> None:
        assert black_player_id != white_player_id != 0, 'player ids can not be the same, and can not be zero'
        self.name = name
        self.board_size, self.stack_history, self.num_to_win = board_size, stack_history, num_to_win
        self.black_player_id, self.white_player_id = black_player_id, white_player_id
        self.black_color, self.white_color = 1, 2
        self.num_actions = board_size ** 2 + 1 if enable_resign else board_size ** 2
        self.resign_action: Optional[int] = self.num_actions - 1 if enable_resign else None
        self.observation_shape = (stack_history * 2 + 1, board_size, board_size)
        self.reset()

    def reset(self, **kwargs) -> np.ndarray:
        n = self.board_size
        self.board = np.zeros((n, n), dtype=np.int8)
        self.actions_mask = np.ones(self.num_actions, dtype=np.bool_)
        self.current_player = self.black_player_id
        self.steps = 0
        self.winner: Optional[int] = None
        self.last_actions = {self.black_player_id: None, self.white_player_id: None}
        # own-stone history planes per player, most recent first (games/env.py:294-310)
        self.feature_planes = {p: np.zeros((self.stack_history, n, n), dtype=np.int8) for p in (self.black_player_id, self.white_player_id)}
        return self.observation()

    # ---- properties (games/env.py:312-365) ----
    @property
    def opponent_player(self) -> int:
        return self.white_player_id if self.current_player == self.black_player_id else self.black_player_id

    @property
    def current_player_color(self) -> int:
        return self.black_color if self.current_player == self.black_player_id else self.white_color

    @property
    def is_board_full(self) -> bool:
        return bool(np.all(self.board != 0))

    @property
    def is_game_over(self) -> bool:
        return self.winner is not None or self.is_board_full

    @property
    def loser(self) -> Optional[int]:
        if self.winner is None:
            return None
        return self.white_player_id if self.winner == self.black_player_id else self.black_player_id

    def action_to_coords(self, action: int) -> Tuple[int, int]:
        return action // self.board_size, action % self.board_size

    def coords_to_action(self, coords: Tuple[int, int]) -> int:
        return coords[0] * self.board_size + coords[1]

    def is_action_valid(self, action: int) -> bool:
        return 0 <= action < self.num_actions and bool(self.actions_mask[action])

    # ---- dynamics ----
    def step(self, action: int):
        """games/env.py:117-154: returns (observation, reward, done, info); the player is not switched on the final move."""
        if not 0 <= action <= self.num_actions - 1:
            raise ValueError(f'Invalid action. Expect action to be in range [0, {self.num_actions}], got {action}')
        if not self.actions_mask[action]:
            raise ValueError(f'Invalid action. The action {action} has alread been taken.')
        if self.is_game_over:
            raise RuntimeError('Game is over, call reset before using step method.')
        action = int(action)
        reward = 0.0
        self.actions_mask[action] = False
        self.last_actions[self.current_player] = action
        if action == self.resign_action:
            reward = -1.0
            self.winner = self.opponent_player
        else:
            r, c = self.action_to_coords(action)
            self.board[r, c] = self.current_player_color
            planes = self.feature_planes[self.current_player]
            planes[1:] = planes[:-1].copy()
            planes[0] = (self.board == self.current_player_color)
            if self.is_current_player_won():
                reward = 1.0
                self.winner = self.current_player
        done = self.is_game_over
        if not done:
            self.current_player = self.opponent_player
        self.steps += 1
        return self.observation(), reward, done, {}

    def is_current_player_won(self) -> bool:
        """Lines through the last move only; needs at least 2 * (num_to_win - 1) earlier plies (steps not yet incremented)."""
        if self.steps < (self.num_to_win - 1) * 2:
            return False
        last = self.last_actions[self.current_player]
        if last is None or last == self.resign_action:
            return False
        r0, c0 = self.action_to_coords(last)
        colour, n = self.current_player_color, self.board_size
        for dr, dc in ((0, 1), (1, 0), (1, 1), (-1, 1)):
            count = 1
            for sgn in (1, -1):
                r, c = r0 + sgn * dr, c0 + sgn * dc
                while 0 <= r < n and 0 <= c < n and self.board[r, c] == colour:
                    count += 1
                    r, c = r + sgn * dr, c + sgn * dc
            if count >= self.num_to_win:
                return True
        return False

    def observation(self) -> np.ndarray:
        """[X_t, Y_t, X_t-1, Y_t-1, ..., C] from the side to move, int8 (games/env.py:242-271)."""
        me, opp = self.current_player, self.opponent_player
        n = self.board_size
        out = np.zeros(self.observation_shape, dtype=np.int8)
        out[0:2 * self.stack_history:2] = self.feature_planes[me]
        out[1:2 * self.stack_history:2] = self.feature_planes[opp]
        out[-1] = 1 if me == self.black_player_id else 0
        return out.reshape(self.observation_shape) if n else out


class TicTacToeEnv(BoardGameEnv):
    """games/tictactoe.py:25-31"""

    def __init__(self, stack_history: int = 4) -> None:
        super().__init__(board_size=3, stack_history=stack_history, num_to_win=3, name='TicTacToe')


class GomokuEnv(BoardGameEnv):
    """games/gomoku.py:25-70"""

    def __init__(self, board_size: int = 15, stack_history: int = 4, num_to_win: int = 5) -> None:
        super().__init__(board_size=board_size, stack_history=stack_history, num_to_win=num_to_win, name='Gomoku')


class ConnectFourEnv(BoardGameEnv):
    """Connect Four; the specification of the device env MZ_ENV_CONNECT4 (`csrc/mz_connect4.h`, same rules).  The reference defines no such
    game: this class is the definition, with `BoardGameEnv`'s conventions wherever they apply.  A `rows` x `cols` board, row `rows - 1` the
    bottom; players 1 (black, moves first) and 2 (white).  Action c < cols drops a stone into column c, where it lands on the lowest empty
    row; action `cols` resigns (reward -1 for the mover, the opponent wins).  A column is legal while its top cell is empty, resign always;
    `step` raises on a full column.  `num_to_win` or more stones of the mover in a line through the stone just placed (horizontal, vertical,
    either diagonal; a line ends at the board's edges) win with reward +1, tested from ply 2 * (num_to_win - 1) on (the family's rule, with
    the pre-increment step count); a win on the last empty cell is a win.  A full board without a win is a draw: reward 0, game over.  The
    side to move switches only if the game is not over.  Observation: `BoardGameEnv.observation`'s planes on (rows, cols)."""

    def __init__(self, rows: int = 6, cols: int = 7, num_to_win: int = 4, stack_history: int = 4) -> None:
        if rows < 1 or cols < 1 or not 2 <= num_to_win <= max(rows, cols) or stack_history < 1:
            raise ValueError('ConnectFourEnv needs rows >= 1, cols >= 1, 2 <= num_to_win <= max(rows, cols) and stack_history >= 1')
        self.name = 'ConnectFour'
        self.rows, self.cols, self.stack_history, self.num_to_win = rows, cols, stack_history, num_to_win
        self.black_player_id, self.white_player_id = 1, 2
        self.black_color, self.white_color = 1, 2
        self.num_actions = cols + 1
        self.resign_action: Optional[int] = cols
        self.observation_shape = (stack_history * 2 + 1, rows, cols)
        self.reset()

    def reset(self, **kwargs) -> np.ndarray:
        self.board = np.zeros((self.rows, self.cols), dtype=np.int8)
        self.actions_mask = np.ones(self.num_actions, dtype=np.bool_)
        self.current_player = self.black_player_id
        self.steps = 0
        self.winner: Optional[int] = None
        self.last_actions = {self.black_player_id: None, self.white_player_id: None}
        self.last_coords: Optional[Tuple[int, int]] = None  # where the last stone landed
        self.feature_planes = {p: np.zeros((self.stack_history, self.rows, self.cols), dtype=np.int8) for p in (self.black_player_id, self.white_player_id)}
        return self.observation()

    def landing_row(self, col: int) -> int:
        """The lowest empty row of column `col` (-1: the column is full)."""
        return int(self.rows - 1 - np.count_nonzero(self.board[:, col]))

    def action_to_coords(self, action: int) -> Tuple[int, int]:
        return self.landing_row(action), action

    def coords_to_action(self, coords: Tuple[int, int]) -> int:
        return coords[1]

    def step(self, action: int):
        if not 0 <= action <= self.num_actions - 1:
            raise ValueError(f'Invalid action. Expect action to be in range [0, {self.num_actions}], got {action}')
        if not self.actions_mask[action]:
            raise ValueError(f'Invalid action. The column {action} is full.')
        if self.is_game_over:
            raise RuntimeError('Game is over, call reset before using step method.')
        action = int(action)
        reward = 0.0
        self.last_actions[self.current_player] = action
        if action == self.resign_action:
            reward = -1.0
            self.winner = self.opponent_player
        else:
            r = self.landing_row(action)
            self.board[r, action] = self.current_player_color
            self.last_coords = (r, action)
            if r == 0:
                self.actions_mask[action] = False  # the top cell is taken
            planes = self.feature_planes[self.current_player]
            planes[1:] = planes[:-1].copy()
            planes[0] = (self.board == self.current_player_color)
            if self.is_current_player_won():
                reward = 1.0
                self.winner = self.current_player
        done = self.is_game_over
        if not done:
            self.current_player = self.opponent_player
        self.steps += 1
        return self.observation(), reward, done, {}

    def is_current_player_won(self) -> bool:
        """Lines through the last stone only; needs at least 2 * (num_to_win - 1) earlier plies (steps not yet incremented)."""
        if self.steps < (self.num_to_win - 1) * 2:
            return False
        last = self.last_actions[self.current_player]
        if last is None or last == self.resign_action:
            return False
        r0, c0 = self.last_coords
        colour = self.current_player_color
        for dr, dc in ((0, 1), (1, 0), (1, 1), (-1, 1)):
            count = 1
            for sgn in (1, -1):
                r, c = r0 + sgn * dr, c0 + sgn * dc
                while 0 <= r < self.rows and 0 <= c < self.cols and self.board[r, c] == colour:
                    count += 1
                    r, c = r + sgn * dr, c + sgn * dc
            if count >= self.num_to_win:
                return True
        return False

    def observation(self) -> np.ndarray:
        me, opp = self.current_player, self.opponent_player
        out = np.zeros(self.observation_shape, dtype=np.int8)
        out[0:2 * self.stack_history:2] = self.feature_planes[me]
        out[1:2 * self.stack_history:2] = self.feature_planes[opp]
        out[-1] = 1 if me == self.black_player_id else 0
        return out


class OthelloEnv(BoardGameEnv):
    """Othello (Reversi); the specification of the device env MZ_ENV_OTHELLO (`csrc/mz_othello.h`, same rules).  The reference defines no
    such game: this class is the definition, with `BoardGameEnv`'s conventions wherever they apply.  A `rows` x `cols` board (each 4..8),
    point r * cols + c; players 1 (black, moves first) and 2 (white); start: white on (r0, c0) and (r0 + 1, c0 + 1), black on (r0, c0 + 1)
    and (r0 + 1, c0) with r0 = rows // 2 - 1, c0 = cols // 2 - 1.  Action a < rows * cols places a stone on point a: legal iff the point
    is empty and the stone flips at least one run -- in each of the 8 directions, one or more opposing stones next to the point followed
    directly by a stone of the mover; runs end at the board's edges.  Action rows * cols passes: legal iff the mover has no placement (a
    real ply: the side to move alternates on every ply).  Action rows * cols + 1 resigns (always legal; -1 for the mover, the opponent
    wins).  After a placement, if neither colour can place, the game is over and the stones are counted after the flips: more for the
    mover +1, fewer -1 (the opponent wins), equal 0 (a draw, no winner).  A pass never ends a game.  The side to move switches only if
    the game is not over, and the mask is rebuilt only then.  Both colours' history planes advance on every ply, pass included: plane k
    of colour p holds p's stones as they stood k plies ago (a fresh game: plane 0 the start stones, the older planes empty).
    Observation: `BoardGameEnv.observation`'s planes on (rows, cols)."""

    DIRECTIONS = ((0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1))

    def __init__(self, rows: int = 8, cols: int = 8, stack_history: int = 4) -> None:
        if not (4 <= rows <= 8 and 4 <= cols <= 8) or stack_history < 1:
            raise ValueError('OthelloEnv needs rows and cols in 4..8 and stack_history >= 1')
        self.name = 'Othello'
        self.rows, self.cols, self.stack_history = rows, cols, stack_history
        self.black_player_id, self.white_player_id = 1, 2
        self.black_color, self.white_color = 1, 2
        self.num_actions = rows * cols + 2
        self.pass_action = rows * cols
        self.resign_action: Optional[int] = rows * cols + 1
        self.observation_shape = (stack_history * 2 + 1, rows, cols)
        self.reset()

    def reset(self, **kwargs) -> np.ndarray:
        self.board = np.zeros((self.rows, self.cols), dtype=np.int8)
        r0, c0 = self.rows // 2 - 1, self.cols // 2 - 1
        self.board[r0, c0] = self.board[r0 + 1, c0 + 1] = self.white_color
        self.board[r0, c0 + 1] = self.board[r0 + 1, c0] = self.black_color
        self.current_player = self.black_player_id
        self.steps = 0
        self.winner: Optional[int] = None
        self.finished = False  # the game ended by the count (a draw has no winner)
        self.last_actions = {self.black_player_id: None, self.white_player_id: None}
        self.feature_planes = {p: np.zeros((self.stack_history, self.rows, self.cols), dtype=np.int8) for p in (self.black_player_id, self.white_player_id)}
        for p in (self.black_player_id, self.white_player_id):
            self.feature_planes[p][0] = (self.board == p)
        self._rebuild_mask()
        return self.observation()

    @property
    def is_game_over(self) -> bool:
        return self.winner is not None or self.finished

    def action_to_coords(self, action: int) -> Tuple[int, int]:
        return action // self.cols, action % self.cols

    def coords_to_action(self, coords: Tuple[int, int]) -> int:
        return coords[0] * self.cols + coords[1]

    def flips(self, r0: int, c0: int, colour: int):
        """The stones a placement of `colour` on the empty point (r0, c0) flips, as a list of coordinates."""
        out = []
        for dr, dc in self.DIRECTIONS:
            run = []
            r, c = r0 + dr, c0 + dc
            while 0 <= r < self.rows and 0 <= c < self.cols and self.board[r, c] == 3 - colour:
                run.append((r, c))
                r, c = r + dr, c + dc
            if run and 0 <= r < self.rows and 0 <= c < self.cols and self.board[r, c] == colour:
                out += run
        return out

    def legal_placements(self, colour: int) -> np.ndarray:
        """bool [rows * cols]: the points on which `colour` may place."""
        out = np.zeros(self.rows * self.cols, dtype=np.bool_)
        for r in range(self.rows):
            for c in range(self.cols):
                if self.board[r, c] == 0 and self.flips(r, c, colour):
                    out[r * self.cols + c] = True
        return out

    def _rebuild_mask(self) -> None:
        nn = self.rows * self.cols
        self.actions_mask = np.zeros(self.num_actions, dtype=np.bool_)
        self.actions_mask[:nn] = self.legal_placements(self.current_player_color)
        self.actions_mask[nn] = not self.actions_mask[:nn].any()
        self.actions_mask[nn + 1] = True

    def step(self, action: int):
        if not 0 <= action <= self.num_actions - 1:
            raise ValueError(f'Invalid action. Expect action to be in range [0, {self.num_actions}], got {action}')
        if not self.actions_mask[action]:
            raise ValueError(f'Invalid action. The action {action} is not legal here.')
        if self.is_game_over:
            raise RuntimeError('Game is over, call reset before using step method.')
        action = int(action)
        reward = 0.0
        me, opp = self.current_player, self.opponent_player
        self.last_actions[me] = action
        if action == self.resign_action:
            reward = -1.0
            self.winner = opp
        else:
            if action != self.pass_action:
                r, c = self.action_to_coords(action)
                for fr, fc in self.flips(r, c, me):
                    self.board[fr, fc] = me
                self.board[r, c] = me
            for p in (me, opp):  # both histories advance on every ply
                planes = self.feature_planes[p]
                planes[1:] = planes[:-1].copy()
                planes[0] = (self.board == p)
            if action != self.pass_action and not self.legal_placements(me).any() and not self.legal_placements(opp).any():
                mine, theirs = int(np.count_nonzero(self.board == me)), int(np.count_nonzero(self.board == opp))
                self.finished = True
                if mine > theirs:
                    reward, self.winner = 1.0, me
                elif mine < theirs:
                    reward, self.winner = -1.0, opp
        done = self.is_game_over
        if not done:
            self.current_player = opp
            self._rebuild_mask()
        self.steps += 1
        return self.observation(), reward, done, {}

    def is_current_player_won(self) -> bool:
        return self.winner is not None and self.winner == self.current_player

    def observation(self) -> np.ndarray:
        me, opp = self.current_player, self.opponent_player
        out = np.zeros(self.observation_shape, dtype=np.int8)
        out[0:2 * self.stack_history:2] = self.feature_planes[me]
        out[1:2 * self.stack_history:2] = self.feature_planes[opp]
        out[-1] = 1 if me == self.black_player_id else 0
        return out


class GoEnv(BoardGameEnv):
    """Go; the specification of the device env MZ_ENV_GO (`csrc/mz_go.h`, same rules).  The reference defines no such game: this class is
    the definition, with `BoardGameEnv`'s conventions wherever they apply.  A `rows` x `cols` board (each 3..19), point r * cols + c, empty
    at the start; players 1 (black, moves first) and 2 (white); nn = rows * cols, nn + 2 actions.  A group is a 4-connected set of stones
    of one colour, a liberty an empty 4-neighbour of one of its stones.
    Placement (action a < nn): the stone goes on the empty point a, then every opposing group without a liberty is removed.  Legal iff the
    point is empty, it is not the ko point, and the mover's group containing the new stone has a liberty after those removals (suicide is
    illegal, a "suicide" that captures is legal).
    Simple ko: if a placement captures exactly one stone and the new stone is a one-stone group with exactly one liberty (the captured
    point), that point is forbidden to the opponent on the next ply only; any ply, a pass included, clears it.  No superko.
    Pass (action nn): always legal, a real ply.  Resign (action nn + 1): -1 for the mover, the opponent wins; legal iff `allow_resign`
    (off: the mask entry is 0 for the whole game).
    End: a resignation; a pass directly after a pass; or the ply that makes steps == max_plies, whatever the action (`max_plies` 0 means
    2 * nn, else 1 <= max_plies <= 2 * nn).  The last two end in a Tromp-Taylor area count: a colour's area is its stones plus every empty
    region whose neighbouring stones are all of that colour (a region touching both colours, or neither, counts for nobody).  Black wins
    iff 2 * black_area > 2 * white_area + komi2 (`komi2`: twice the komi, an integer in 0 .. 2 * nn), white iff it is less, equal is a draw
    without a winner; the final mover gets +1, -1 or 0.
    Both colours' history planes advance on every ply, pass included (plane k of colour p: p's stones as they stood k plies ago).  The side
    to move switches, and the mask is rebuilt, only if the game goes on.  Observation: `BoardGameEnv.observation`'s planes on (rows,
    cols); ko and the pass flag are not planes, the history carries them."""

    def __init__(self, rows: int = 9, cols: int = 9, komi2: int = 15, max_plies: int = 0, allow_resign: bool = True, stack_history: int = 4) -> None:
        if not (3 <= rows <= 19 and 3 <= cols <= 19) or stack_history < 1:
            raise ValueError('GoEnv needs rows and cols in 3..19 and stack_history >= 1')
        nn = rows * cols
        if not 0 <= komi2 <= 2 * nn:
            raise ValueError(f'GoEnv needs 0 <= komi2 <= 2 * rows * cols, got {komi2}')
        if not 0 <= max_plies <= 2 * nn:
            raise ValueError(f'GoEnv needs max_plies = 0 (2 * rows * cols) or 1 <= max_plies <= 2 * rows * cols, got {max_plies}')
        self.name = 'Go'
        self.rows, self.cols, self.stack_history = rows, cols, stack_history
        self.komi2, self.max_plies, self.allow_resign = int(komi2), int(max_plies) if max_plies else 2 * nn, bool(allow_resign)
        self.black_player_id, self.white_player_id = 1, 2
        self.black_color, self.white_color = 1, 2
        self.num_actions = nn + 2
        self.pass_action = nn
        self.resign_action: Optional[int] = nn + 1
        self.observation_shape = (stack_history * 2 + 1, rows, cols)
        self.reset()

    def reset(self, **kwargs) -> np.ndarray:
        self.board = np.zeros((self.rows, self.cols), dtype=np.int8)
        self.current_player = self.black_player_id
        self.steps = 0
        self.winner: Optional[int] = None
        self.finished = False  # the game ended by the count (a draw has no winner)
        self.ko_point: Optional[int] = None  # forbidden to the side to move on this ply
        self.last_was_pass = False
        self.last_actions = {self.black_player_id: None, self.white_player_id: None}
        self.feature_planes = {p: np.zeros((self.stack_history, self.rows, self.cols), dtype=np.int8) for p in (self.black_player_id, self.white_player_id)}
        self._rebuild_mask()
        return self.observation()

    @property
    def is_game_over(self) -> bool:
        return self.winner is not None or self.finished

    def action_to_coords(self, action: int) -> Tuple[int, int]:
        return action // self.cols, action % self.cols

    def coords_to_action(self, coords: Tuple[int, int]) -> int:
        return coords[0] * self.cols + coords[1]

    def neighbours(self, r: int, c: int):
        return [(r + dr, c + dc) for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1)) if 0 <= r + dr < self.rows and 0 <= c + dc < self.cols]

    @staticmethod
    def group_of(board: np.ndarray, r0: int, c0: int):
        """(stones, liberties) of the group of the stone on (r0, c0) of `board`, as sets of coordinates."""
        rows, cols = board.shape
        colour = board[r0, c0]
        stones, libs, todo = {(r0, c0)}, set(), [(r0, c0)]
        while todo:
            r, c = todo.pop()
            for q in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                if not (0 <= q[0] < rows and 0 <= q[1] < cols):
                    continue
                if board[q] == 0:
                    libs.add(q)
                elif board[q] == colour and q not in stones:
                    stones.add(q)
                    todo.append(q)
        return stones, libs

    @classmethod
    def all_groups_have_liberty(cls, board: np.ndarray) -> bool:
        """Whether `board` (any shape) is a legal Go position: every group has a liberty."""
        return all(cls.group_of(board, r, c)[1] for r, c in zip(*np.nonzero(board)))

    def try_place(self, board: np.ndarray, r: int, c: int, colour: int):
        """A placement of `colour` on the empty point (r, c) of `board`, ko aside: (board after, captured points, ko point it creates or
        None), or None if it is suicide."""
        b = board.copy()
        b[r, c] = colour
        captured = []
        for q in self.neighbours(r, c):
            if b[q] == 3 - colour:
                stones, libs = self.group_of(b, *q)
                if not libs:
                    for s in stones:
                        b[s] = 0
                    captured += sorted(stones)
        stones, libs = self.group_of(b, r, c)
        if not libs:
            return None
        ko = self.coords_to_action(captured[0]) if len(captured) == 1 and len(stones) == 1 and len(libs) == 1 else None
        return b, captured, ko

    def legal_placements(self, colour: int) -> np.ndarray:
        """bool [rows * cols]: the points on which `colour` may place now (the ko point excluded)."""
        out = np.zeros(self.rows * self.cols, dtype=np.bool_)
        for r in range(self.rows):
            for c in range(self.cols):
                a = r * self.cols + c
                if self.board[r, c] != 0 or a == self.ko_point:
                    continue
                # a stone next to an empty point has a liberty whatever it captures; otherwise play it out
                out[a] = any(self.board[q] == 0 for q in self.neighbours(r, c)) or self.try_place(self.board, r, c, colour) is not None
        return out

    def _rebuild_mask(self) -> None:
        nn = self.rows * self.cols
        self.actions_mask = np.zeros(self.num_actions, dtype=np.bool_)
        self.actions_mask[:nn] = self.legal_placements(self.current_player_color)
        self.actions_mask[nn] = True
        self.actions_mask[nn + 1] = self.allow_resign

    def areas(self) -> Tuple[int, int]:
        """Tromp-Taylor areas (black, white): stones plus the empty regions that touch stones of that colour only."""
        area = [0, int(np.count_nonzero(self.board == 1)), int(np.count_nonzero(self.board == 2))]
        seen = np.zeros((self.rows, self.cols), dtype=np.bool_)
        for r0 in range(self.rows):
            for c0 in range(self.cols):
                if self.board[r0, c0] != 0 or seen[r0, c0]:
                    continue
                seen[r0, c0] = True
                region, touches, todo = 0, set(), [(r0, c0)]
                while todo:
                    r, c = todo.pop()
                    region += 1
                    for q in self.neighbours(r, c):
                        if self.board[q] != 0:
                            touches.add(int(self.board[q]))
                        elif not seen[q]:
                            seen[q] = True
                            todo.append(q)
                if len(touches) == 1:
                    area[touches.pop()] += region
        return area[1], area[2]

    def step(self, action: int):
        if not 0 <= action <= self.num_actions - 1:
            raise ValueError(f'Invalid action. Expect action to be in range [0, {self.num_actions}], got {action}')
        if not self.actions_mask[action]:
            raise ValueError(f'Invalid action. The action {action} is not legal here.')
        if self.is_game_over:
            raise RuntimeError('Game is over, call reset before using step method.')
        action = int(action)
        reward = 0.0
        me, opp = self.current_player, self.opponent_player
        self.last_actions[me] = action
        if action == self.resign_action:
            reward = -1.0
            self.winner = opp
        else:
            passed = action == self.pass_action
            self.ko_point = None  # any ply clears it
            if not passed:
                self.board, _, self.ko_point = self.try_place(self.board, *self.action_to_coords(action), me)
            for p in (me, opp):  # both histories advance on every ply
                planes = self.feature_planes[p]
                planes[1:] = planes[:-1].copy()
                planes[0] = (self.board == p)
            if (passed and self.last_was_pass) or self.steps + 1 == self.max_plies:
                black, white = self.areas()
                self.finished = True
                diff = 2 * black - 2 * white - self.komi2  # > 0: black wins
                if diff != 0:
                    self.winner = self.black_player_id if diff > 0 else self.white_player_id
                    reward = 1.0 if self.winner == me else -1.0
            self.last_was_pass = passed
        done = self.is_game_over
        if not done:
            self.current_player = opp
            self._rebuild_mask()
        self.steps += 1
        return self.observation(), reward, done, {}

    def is_current_player_won(self) -> bool:
        return self.winner is not None and self.winner == self.current_player

    def observation(self) -> np.ndarray:
        me, opp = self.current_player, self.opponent_player
        out = np.zeros(self.observation_shape, dtype=np.int8)
        out[0:2 * self.stack_history:2] = self.feature_planes[me]
        out[1:2 * self.stack_history:2] = self.feature_planes[opp]
        out[-1] = 1 if me == self.black_player_id else 0
        return out


class ScaledFloatFrame:
    """`gym_env.py:214-224`: frames as float32 scaled to [0, 1] (x / 255).  Host-stepped self-play with device frame stacking
    recognises it inside `StackFrameAndAction` and uploads the raw uint8 frames instead, scaled on the device to the same values."""

    def __init__(self, env) -> None:
        self.env = env

    def __getattr__(self, name):
        return getattr(self.env, name)

    @staticmethod
    def observation(observation) -> np.ndarray:
        return np.array(observation).astype(np.float32) / 255.0

    def reset(self, **kwargs) -> np.ndarray:
        return self.observation(self.env.reset(**kwargs))

    def step(self, action):
        obs, reward, done, info = self.env.step(action)
        return self.observation(obs), reward, done, info


class StackFrameAndAction:
    """`gym_env.py:271-353`: stacks the last `stack_history` observations, newest first, each with the action that led to it
    as a bias value (action + 1) / num_actions (reset fills every slot with the first observation and action 0).  Vector
    observations [D] become [stack, D + 1]; channel-first images [C, H, W] become [stack * (C + 1), H, W] with the action
    broadcast to a plane.  `env` needs reset() -> obs, step(a) -> (obs, reward, done, info), `observation_shape` and
    `num_actions`."""

    def __init__(self, env, stack_history: int, is_obs_image: bool = False) -> None:
        self.env, self.stack_history, self.is_obs_image = env, stack_history, is_obs_image
        self.num_actions = env.num_actions
        shp = tuple(env.observation_shape)
        self.old_obs_shape = shp[1:] if is_obs_image else shp
        self.observation_shape = (stack_history * (shp[0] + 1),) + shp[1:] if is_obs_image else (stack_history, shp[0] + 1)
        self._obs, self._act = [], []

    def __getattr__(self, name):
        return getattr(self.env, name)

    def _plane(self, action) -> np.ndarray:
        scaled = (action + 1) / self.num_actions
        return scaled * np.ones(self.old_obs_shape if self.is_obs_image else (1,)).astype(np.float32)

    def observation(self) -> np.ndarray:
        obs = np.stack(self._obs, axis=0).astype(np.float32)
        act = np.stack(self._act, axis=0).astype(np.float32)
        if self.is_obs_image:
            return np.concatenate([obs.reshape((-1,) + obs.shape[2:]), act], axis=0)
        return np.concatenate([obs, act], axis=1)

    def reset(self, **kwargs) -> np.ndarray:
        first = self.env.reset(**kwargs)
        self._obs = [first] * self.stack_history
        self._act = [self._plane(0)] * self.stack_history
        return self.observation()

    def step(self, action):
        obs, reward, done, info = self.env.step(action)
        self._obs = [obs] + self._obs[:-1]
        self._act = [self._plane(action)] + self._act[:-1]
        return self.observation(), reward, done, info


class PlayerIdAndActionMaskWrapper:
    """`gym_env.py:356-365`: single-player environments present player ids 1 / 1 and an all-legal action mask."""

    def __init__(self, env) -> None:
        self.env = env
        self.current_player = self.opponent_player = 1
        self.actions_mask = np.ones(env.num_actions, dtype=np.bool_).flatten()

    def __getattr__(self, name):
        return getattr(self.env, name)

    def reset(self, **kwargs):
        return self.env.reset(**kwargs)

    def step(self, action):
        return self.env.step(action)


class _CartPolePhysics:
    """gym 0.23.1 CartPole-v1 (an un-vendored dependency of the reference; its published equations): float64 state, float32
    observation, reward 1 per step, failure beyond |x| 2.4 or |theta| 12 degrees, TimeLimit 500."""

    num_actions = 2
    observation_shape = (4,)

    def __init__(self, seed: int = 1) -> None:
        self._rs = np.random.RandomState(seed)
        self.state, self.steps, self.done = np.zeros(4), 0, True

    def reset(self, state=None) -> np.ndarray:
        self.state = np.asarray(state, np.float64).copy() if state is not None else self._rs.uniform(-0.05, 0.05, size=4)
        self.steps, self.done = 0, False
        return self.state.astype(np.float32)

    def step(self, action: int):
        if self.done:
            raise RuntimeError('Episode is over, call reset before using step method.')
        if action not in (0, 1):
            raise ValueError(f'Invalid action {action}')
        gravity, masscart, masspole, length, force_mag, tau = 9.8, 1.0, 0.1, 0.5, 10.0, 0.02
        total_mass, polemass_length = masspole + masscart, masspole * length
        x, x_dot, theta, theta_dot = self.state
        force = force_mag if action == 1 else -force_mag
        costheta, sintheta = np.cos(theta), np.sin(theta)
        temp = (force + polemass_length * theta_dot * theta_dot * sintheta) / total_mass
        thetaacc = (gravity * sintheta - costheta * temp) / (length * (4.0 / 3.0 - masspole * costheta * costheta / total_mass))
        xacc = temp - polemass_length * thetaacc * costheta / total_mass
        x, x_dot = x + tau * x_dot, x_dot + tau * xacc
        theta, theta_dot = theta + tau * theta_dot, theta_dot + tau * thetaacc
        self.state = np.array([x, x_dot, theta, theta_dot], np.float64)
        self.steps += 1
        failed = x < -2.4 or x > 2.4 or theta < -12 * 2 * np.pi / 360 or theta > 12 * 2 * np.pi / 360
        self.done = bool(failed or self.steps >= 500)
        return self.state.astype(np.float32), 1.0, self.done, {}


class CartPoleEnv(PlayerIdAndActionMaskWrapper):
    """Host-side CartPole-v1 as the reference's `create_classic_environment('CartPole-v1', stack_history=4)` presents it
    (`gym_env.py:436-459`): the physics above inside StackFrameAndAction(stack_history, is_obs_image=False) inside
    PlayerIdAndActionMaskWrapper.  Same rules as the device environment in `csrc/mz_env.h`; for evaluators and tools."""

    def __init__(self, stack_history: int = 4, seed: int = 1) -> None:
        super().__init__(StackFrameAndAction(_CartPolePhysics(seed), stack_history, False))
        self.stack_history = stack_history
        self.reset()

    def reset(self, state=None) -> np.ndarray:
        return self.env.reset(state=state)


class CatchEnv:
    """Catch (as in bsuite) rendered as an image; the specification of the device env MZ_ENV_CATCH (`csrc/mz_catch.h`, same rules).
    A `rows` x `cols` grid of `cell_h` x `cell_w` pixel cells on a uint8 frame [1, rows * cell_h, cols * cell_w].  The ball sits at
    (br, bc), the paddle at column pc of the last row.  reset: br = `start_row`, bc = the `ball_col` given (else the next of `ball_cols`,
    else a draw from the env's own RandomState), pc = cols // 2.  step(a), a in (0 left, 1 stay, 2 right): pc = clip(pc + a - 1, 0,
    cols - 1), then br += 1; when br == rows - 1 the episode is done with reward +1.0 if bc == pc, else -1.0; every other reward is 0.
    The frame is 0 with every pixel of the ball's cell and of the paddle's cell 255.  `first_row`: the ball's row in the first episode
    only (the device env staggers its envs this way); `ball_cols`: an iterable of ball columns for successive resets."""

    name = 'Catch'
    num_actions = 3

    def __init__(self, rows: int = 12, cols: int = 12, cell_h: int = 8, cell_w: int = 8, start_row: int = 0, seed: int = 1, ball_cols=None,
                 first_row: Optional[int] = None) -> None:
        if rows < 2 or cols < 1 or cell_h < 1 or cell_w < 1 or not 0 <= start_row <= rows - 2:
            raise ValueError('CatchEnv needs rows >= 2, cols >= 1, cells of at least one pixel and 0 <= start_row <= rows - 2')
        if first_row is not None and not 0 <= first_row <= rows - 2:
            raise ValueError('first_row must be a row above the paddle\'s')
        self.rows, self.cols, self.cell_h, self.cell_w, self.start_row = rows, cols, cell_h, cell_w, start_row
        self.observation_shape = (1, rows * cell_h, cols * cell_w)
        self.max_episode_steps = rows - 1
        self._rs = np.random.RandomState(seed)
        self._cols = None if ball_cols is None else iter(ball_cols)
        self._first_row = first_row
        self.br = self.bc = self.pc = 0
        self.done = True

    def reset(self, ball_col: Optional[int] = None) -> np.ndarray:
        if ball_col is None:
            ball_col = next(self._cols) if self._cols is not None else self._rs.randint(self.cols)
        if not 0 <= ball_col < self.cols:
            raise ValueError(f'ball column {ball_col} outside the {self.cols} columns')
        self.br, self._first_row = (self.start_row if self._first_row is None else self._first_row), None
        self.bc, self.pc, self.done = int(ball_col), self.cols // 2, False
        return self.render()

    def step(self, action: int):
        if self.done:
            raise RuntimeError('Episode is over, call reset before using step method.')
        if action not in (0, 1, 2):
            raise ValueError(f'Invalid action {action}')
        self.pc = min(max(self.pc + int(action) - 1, 0), self.cols - 1)
        self.br += 1
        reward = 0.0
        if self.br == self.rows - 1:
            self.done = True
            reward = 1.0 if self.bc == self.pc else -1.0
        return self.render(), reward, self.done, {}

    def render(self) -> np.ndarray:
        h, w = self.cell_h, self.cell_w
        frame = np.zeros(self.observation_shape, np.uint8)
        frame[0, self.br * h:(self.br + 1) * h, self.bc * w:(self.bc + 1) * w] = 255
        frame[0, (self.rows - 1) * h:, self.pc * w:(self.pc + 1) * w] = 255
        return frame


def make_catch_env(rows: int = 12, cols: int = 12, cell_h: int = 8, cell_w: int = 8, stack_history: int = 4, **kwargs):
    """`CatchEnv` as the Atari nets see it: PlayerIdAndActionMaskWrapper(StackFrameAndAction(ScaledFloatFrame(env), stack_history, True)),
    observations float32 [2 * stack_history, rows * cell_h, cols * cell_w]."""
    return PlayerIdAndActionMaskWrapper(StackFrameAndAction(ScaledFloatFrame(CatchEnv(rows, cols, cell_h, cell_w, **kwargs)), stack_history, True))


def catch_random_policy_return(rows: int = 12, cols: int = 12, start_row: int = 0) -> float:
    """The expected return of the uniformly random policy on `CatchEnv`, exactly: dynamic programming over (paddle column, steps left)
    for every ball column, averaged over the ball columns (each equally likely)."""
    steps = rows - 1 - start_row
    total = 0.0
    for bc in range(cols):
        v = np.where(np.arange(cols) == bc, 1.0, -1.0)  # the value with no step left: the catch test
        for _ in range(steps):
            left, right = np.concatenate([v[:1], v[:-1]]), np.concatenate([v[1:], v[-1:]])  # (clipped at the walls)
            v = (left + v + right) / 3.0
        total += v[cols // 2]
    return float(total / cols)


class BreakoutEnv:
    """A brick-breaking game rendered as an image; the specification of the device env MZ_ENV_BREAKOUT (`csrc/mz_breakout.h`, same rules).
    A `rows` x `cols` grid (cols <= 32) of `cell_h` x `cell_w` pixel cells on a uint8 frame [1, rows * cell_h, cols * cell_w].  Bricks fill
    rows 1 .. K (`brick_rows`, 1 to 3; one bitmask per row, bit c = column c), row 0 is empty, the paddle lives in row rows - 1.  The ball
    at (bx, by) moves diagonally, direction d in (0 up-left, 1 up-right, 2 down-right, 3 down-left).

    reset with start code k in 0 .. 2 cols - 1 (the `start_code` given, else the next of `start_codes`, else a draw from the env's own
    RandomState): bx = k >> 1, by = K + 1, d = 2 + (k & 1), px = cols // 2, trail (lx, ly) = (bx, by), all bricks, t = 0.

    step(a), a in (0 left, 1 stay, 2 right), in this order: px = clip(px + a - 1, 0, cols - 1); (nx, ny) = (bx, by) + delta[d]; nx off the
    grid is clamped and d flips horizontally; then exactly one of: ny < 0 -> ny = 0, d flips vertically | a brick at (ny, nx) -> it is
    removed, reward 1, ny = by, d flips vertically | ny == rows - 1 -> first the bricks are refilled if none is left, then bx == px: d flips
    vertically, ny = by; else nx == px: d flips both ways, ny = by; else the episode ends with reward 0 | nothing.  Then the trail becomes
    the old ball cell, the ball moves, t += 1, and t == max_moves ends the episode (a brick reward and the cap may fall on one move).

    Frame: background 0, bricks 96, trail cell 64, paddle cell 160, ball cell 255; where cells coincide ball > paddle > trail > brick."""

    name = 'Breakout'
    num_actions = 3
    DX, DY = (-1, 1, 1, -1), (-1, -1, 1, 1)
    FLIPX, FLIPY, FLIPBOTH = (1, 0, 3, 2), (3, 2, 1, 0), (2, 3, 0, 1)
    BRICK, TRAIL, PADDLE, BALL = 96, 64, 160, 255

    def __init__(self, rows: int = 12, cols: int = 12, cell_h: int = 8, cell_w: int = 8, brick_rows: int = 3, max_moves: int = 200, seed: int = 1,
                 start_codes=None) -> None:
        if not 1 <= brick_rows <= 3 or rows < brick_rows + 3 or not 3 <= cols <= 32 or cell_h < 1 or cell_w < 1 or max_moves < 1:
            raise ValueError('BreakoutEnv needs brick_rows in 1..3, rows >= brick_rows + 3, 3 <= cols <= 32, cells of at least one pixel and max_moves >= 1')
        self.rows, self.cols, self.cell_h, self.cell_w, self.brick_rows, self.max_moves = rows, cols, cell_h, cell_w, brick_rows, max_moves
        self.observation_shape = (1, rows * cell_h, cols * cell_w)
        self.max_episode_steps = max_moves
        self._rs = np.random.RandomState(seed)
        self._codes = None if start_codes is None else iter(start_codes)
        self.bx = self.by = self.d = self.px = self.lx = self.ly = self.t = 0
        self.bricks = [0] * brick_rows
        self.done = True

    def reset(self, start_code: Optional[int] = None) -> np.ndarray:
        if start_code is None:
            start_code = next(self._codes) if self._codes is not None else self._rs.randint(2 * self.cols)
        if not 0 <= start_code < 2 * self.cols:
            raise ValueError(f'start code {start_code} outside 0 .. {2 * self.cols - 1}')
        k = int(start_code)
        self.bx, self.by, self.d, self.px = k >> 1, self.brick_rows + 1, 2 + (k & 1), self.cols // 2
        self.lx, self.ly, self.t, self.done = self.bx, self.by, 0, False
        self.bricks = [(1 << self.cols) - 1] * self.brick_rows
        return self.render()

    def step(self, action: int):
        if self.done:
            raise RuntimeError('Episode is over, call reset before using step method.')
        if action not in (0, 1, 2):
            raise ValueError(f'Invalid action {action}')
        self.px = min(max(self.px + int(action) - 1, 0), self.cols - 1)
        d = self.d
        nx, ny, reward = self.bx + self.DX[d], self.by + self.DY[d], 0.0
        if nx < 0 or nx > self.cols - 1:
            nx, d = min(max(nx, 0), self.cols - 1), self.FLIPX[d]
        if ny < 0:
            ny, d = 0, self.FLIPY[d]
        elif 1 <= ny <= self.brick_rows and (self.bricks[ny - 1] >> nx) & 1:
            self.bricks[ny - 1] &= ~(1 << nx)
            reward, ny, d = 1.0, self.by, self.FLIPY[d]
        elif ny == self.rows - 1:
            if not any(self.bricks):
                self.bricks = [(1 << self.cols) - 1] * self.brick_rows
            if self.bx == self.px:
                d, ny = self.FLIPY[d], self.by
            elif nx == self.px:
                d, ny = self.FLIPBOTH[d], self.by
            else:
                self.done = True
        self.lx, self.ly, self.bx, self.by, self.d = self.bx, self.by, nx, ny, d
        self.t += 1
        if self.t == self.max_moves:
            self.done = True
        return self.render(), reward, self.done, {}

    def render(self) -> np.ndarray:
        h, w = self.cell_h, self.cell_w
        frame = np.zeros(self.observation_shape, np.uint8)

        def paint(r, c, v):
            frame[0, r * h:(r + 1) * h, c * w:(c + 1) * w] = v

        for k, m in enumerate(self.bricks):
            for c in range(self.cols):
                if (m >> c) & 1:
                    paint(k + 1, c, self.BRICK)
        paint(self.ly, self.lx, self.TRAIL)
        paint(self.rows - 1, self.px, self.PADDLE)
        paint(self.by, self.bx, self.BALL)
        return frame


def make_breakout_env(rows: int = 12, cols: int = 12, cell_h: int = 8, cell_w: int = 8, stack_history: int = 4, **kwargs):
    """`BreakoutEnv` as the Atari nets see it: PlayerIdAndActionMaskWrapper(StackFrameAndAction(ScaledFloatFrame(env), stack_history, True)),
    observations float32 [2 * stack_history, rows * cell_h, cols * cell_w]."""
    return PlayerIdAndActionMaskWrapper(StackFrameAndAction(ScaledFloatFrame(BreakoutEnv(rows, cols, cell_h, cell_w, **kwargs)), stack_history, True))


BREAKOUT_STREAM = 0x71000000  # the start code's Philox stream (mz_breakout.h BREAKOUT_STREAM)


def _philox_uniform(seed: int, c1: int, c2: int, c3: int) -> float:
    """The first double of the device stream Philox(seed, c1, c2, c3) (Philox4x32-10 as `csrc/mz_device.h` keys it: counter (0, c1, c2,
    c3), key (seed low, seed high); uniform = ((r0 >> 5) * 2^26 + (r1 >> 6)) / 2^53)."""
    M = 0xFFFFFFFF
    c = [0, c1 & M, c2 & M, c3 & M]
    k0, k1 = seed & M, (seed >> 32) & M
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> 32) ^ c[3] ^ k1) & M, p0 & M]
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return ((c[0] >> 5) * 67108864.0 + (c[1] >> 6)) / 9007199254740992.0


def breakout_start_code(seed: int, env: int, episode: int, cols: int) -> int:
    """The start code the device Breakout env draws for episode `episode` of env `env` in self-play on a planner seeded `seed`:
    min(2 cols - 1, floor(u * 2 cols)), u the first double of Philox(seed, env, episode, 0x71000000)."""
    return min(2 * cols - 1, int(np.floor(_philox_uniform(int(seed), int(env), int(episode), BREAKOUT_STREAM) * (2 * cols))))


def breakout_track_action(env) -> int:
    """The scripted policy that tracks the ball: move the paddle towards the column the ball is in (a `BreakoutEnv`, or a wrapper of one)."""
    return 1 + int(np.sign(env.bx - env.px))
