"""Cases for the device Breakout env (MZ_ENV_BREAKOUT, csrc/mz_breakout.h): a numpy model of what the device does -- games.BreakoutEnv's rules
on per-env state arrays for B envs at once, the start code's Philox draw, the restart of a finished env, and the renderer in the kernel's own
form (flat byte array, one 16-byte run per lane, one division and then counters) -- the scripted episodes with their expected states written
out by hand, and the shapes.  tests/test_breakout_host.py holds the model to games.BreakoutEnv frame for frame (and shows that each planted
mistake is seen by a named case); tests/test_gpu_breakout.py holds the device to host BreakoutEnv objects fed by `start_code`."""
import numpy as np

from helpers import philox_uniforms

STREAM = 0x71000000  # the start code's Philox stream (mz_breakout.h BREAKOUT_STREAM)
BRICK, TRAIL, PADDLE, BALL = 96, 64, 160, 255

# name -> (rows, cols, cell_h, cell_w, brick_rows, max_moves): the frame is [1, rows * cell_h, cols * cell_w]
SHAPES = {
    'g43': (4, 3, 3, 4, 1, 12),       # 12 x 12 frames; the smallest grid that reaches every branch
    'g43px': (4, 3, 1, 1, 1, 12),     # 4 x 3 frames of one-pixel cells: 12 bytes per env, every run crosses envs
    'g65': (6, 5, 2, 3, 2, 200),      # 12 x 15 frames: cell width 3 (no multiple of 4), frame size 180 (no multiple of 16)
    'g68': (6, 8, 2, 3, 2, 200),      # 12 x 24 frames, cell width 3
    'g32': (8, 32, 1, 1, 3, 200),     # 8 x 32 frames: the brick masks' top bit, runs that span 16 cells
    'atari': (12, 12, 8, 8, 3, 200),  # 96 x 96, the Atari nets' frame
}

BUGS = ('paddle_after_ball', 'flip_swapped', 'ball_into_brick_row', 'refill_after_paddle', 'trail_stale', 'paint_reversed', 'cap_off_by_one',
        'start_dir_dropped', 'bit31_lost')
# the named case (SCRIPTS / 'wide32') on which each planted mistake must show
SEEN_BY = {'paddle_after_ball': 'side_bounce', 'flip_swapped': 'miss', 'ball_into_brick_row': 'brick_hit', 'refill_after_paddle': 'refill',
           'trail_stale': 'top_bounce', 'paint_reversed': 'paddle_straight', 'cap_off_by_one': 'cap', 'start_dir_dropped': 'miss',
           'bit31_lost': 'wide32'}

DX, DY = (-1, 1, 1, -1), (-1, -1, 1, 1)
FLIPX, FLIPY, FLIPBOTH = (1, 0, 3, 2), (3, 2, 1, 0), (2, 3, 0, 1)


def start_code(seed, e, k, cols):
    """The start code of env e, episode k."""
    u = philox_uniforms(seed, e, k, STREAM, 1)[0]
    return min(2 * cols - 1, int(np.floor(u * 2 * cols)))


class BreakoutModel:
    """B device Breakout envs: the state arrays of mz_breakout.h and its renderer.  `codes`: start codes per env for successive episodes
    (a list of lists; default: the Philox draws of `seed`).  `restart` False: a finished env is frozen as it was (the arena).  `bug` plants
    one mistake (BUGS)."""

    def __init__(self, B, rows, cols, cell_h, cell_w, brick_rows, max_moves, seed=0, codes=None, bug=None, restart=True):
        assert bug is None or bug in BUGS
        self.B, self.rows, self.cols, self.ch, self.cw, self.K, self.cap = B, rows, cols, cell_h, cell_w, brick_rows, max_moves
        self.seed, self.bug, self.codes, self.restart = seed, bug, codes, restart
        self.episode = np.zeros(B, np.int64)
        self.live = np.ones(B, bool)
        z = lambda: np.zeros(B, np.int64)  # noqa: E731
        self.bx, self.by, self.d, self.px, self.lx, self.ly, self.t = z(), z(), z(), z(), z(), z(), z()
        self.bricks = np.zeros((3, B), np.uint32)
        for e in range(B):
            self._start(e)

    def _full(self):
        full = (1 << self.cols) - 1
        return np.uint32(full & 0x7fffffff if self.bug == 'bit31_lost' else full)

    def _start(self, e):
        k = int(self.episode[e])
        code = self.codes[e][k] if self.codes is not None else start_code(self.seed, e, k, self.cols)
        self.bx[e], self.by[e], self.px[e] = code >> 1, self.K + 1, self.cols // 2
        self.d[e] = 2 if self.bug == 'start_dir_dropped' else 2 + (code & 1)
        self.lx[e], self.ly[e], self.t[e] = self.bx[e], self.by[e], 0
        for r in range(3):
            self.bricks[r, e] = self._full() if r < self.K else 0

    def step(self, actions):
        """-> (reward float32 [B], done uint8 [B]); a finished env is at its next episode's reset state afterwards (restart) or frozen."""
        reward, done = np.zeros(self.B, np.float32), np.zeros(self.B, np.uint8)
        flipx, flipy = (FLIPY, FLIPX) if self.bug == 'flip_swapped' else (FLIPX, FLIPY)
        for e in range(self.B):
            if not self.live[e]:
                continue
            old_px = int(self.px[e])
            px = min(max(old_px + int(actions[e]) - 1, 0), self.cols - 1)
            test_px = old_px if self.bug == 'paddle_after_ball' else px
            bx, by, d = int(self.bx[e]), int(self.by[e]), int(self.d[e])
            br = [int(self.bricks[r, e]) for r in range(3)]
            nx, ny, fin = bx + DX[d], by + DY[d], False
            if nx < 0 or nx > self.cols - 1:
                nx, d = min(max(nx, 0), self.cols - 1), flipx[d]
            if ny < 0:
                ny, d = 0, flipy[d]
            elif 1 <= ny <= self.K and (br[ny - 1] >> nx) & 1:
                br[ny - 1] &= ~(1 << nx)
                reward[e], d = 1.0, flipy[d]
                if self.bug != 'ball_into_brick_row':
                    ny = by
            elif ny == self.rows - 1:
                if self.bug != 'refill_after_paddle' and not any(br):
                    br = [int(self._full()) if r < self.K else 0 for r in range(3)]
                if bx == test_px:
                    d, ny = flipy[d], by
                elif nx == test_px:
                    d, ny = FLIPBOTH[d], by
                elif self.bug == 'refill_after_paddle' and not any(br):  # (the refill as the chain's next alternative: a bounce refills nothing)
                    br = [int(self._full()) if r < self.K else 0 for r in range(3)]
                else:
                    fin = True
            t = int(self.t[e]) + 1
            if t == self.cap + (1 if self.bug == 'cap_off_by_one' else 0):
                fin = True
            done[e] = 1 if fin else 0
            if fin:
                if self.restart:
                    self.episode[e] += 1
                    self._start(e)
                else:
                    self.live[e] = False
                continue
            if self.bug != 'trail_stale':
                self.lx[e], self.ly[e] = bx, by
            self.px[e], self.bx[e], self.by[e], self.d[e], self.t[e] = px, nx, ny, d, t
            for r in range(3):
                self.bricks[r, e] = br[r]
        return reward, done

    def _cell(self, e, cy, cx):
        levels = [(cy == self.by[e] and cx == self.bx[e], BALL), (cy == self.rows - 1 and cx == self.px[e], PADDLE),
                  (cy == self.ly[e] and cx == self.lx[e], TRAIL), (1 <= cy <= 3 and (int(self.bricks[min(max(cy - 1, 0), 2), e]) >> cx) & 1, BRICK)]
        for hit, v in (reversed(levels) if self.bug == 'paint_reversed' else levels):
            if hit:
                return v
        return 0

    def frames(self):
        """uint8 [B, 1, H, W], painted as k_game_render paints: lane i owns bytes 16 i .. 16 i + 15 of the flat array [pad16(B * FE)]; it
        divides once for its first byte and walks the others with counters."""
        H, W = self.rows * self.ch, self.cols * self.cw
        FE, total = H * W, self.B * H * W
        flat = np.zeros((total + 15) // 16 * 16, np.uint8)
        for i0 in range(0, total, 16):
            e, j = divmod(i0, FE)
            row, col = divmod(j, W)
            cy, ry = divmod(row, self.ch)
            cx, rx = divmod(col, self.cw)
            for q in range(16):
                flat[i0 + q] = self._cell(e, cy, cx) if e < self.B else 0
                rx += 1
                if rx == self.cw:
                    rx, cx = 0, cx + 1
                col += 1
                if col == W:
                    col = cx = rx = 0
                    row, ry = row + 1, ry + 1
                    if ry == self.ch:
                        ry, cy = 0, cy + 1
                    if row == H:
                        row = cy = ry = 0
                        e += 1
        assert not flat[total:].any()
        return flat[:total].reshape(self.B, 1, H, W)


def host_envs(B, shape, seed, episodes=64, codes=None):
    """B games.BreakoutEnv objects that play what the device plays: the regenerated start codes (or `codes[e]`)."""
    from muzero_amd.games import BreakoutEnv

    rows, cols, ch, cw, K, cap = shape
    return [BreakoutEnv(rows, cols, ch, cw, brick_rows=K, max_moves=cap,
                        start_codes=codes[e] if codes is not None else [start_code(seed, e, k, cols) for k in range(episodes)]) for e in range(B)]


def play_model(model, actions):
    """-> (frames [moves + 1, B, 1, H, W], rewards [moves, B], dones [moves, B])"""
    frames, rewards, dones = [model.frames()], [], []
    for a in actions:
        r, d = model.step(a)
        frames.append(model.frames())
        rewards.append(r)
        dones.append(d)
    return np.stack(frames), np.stack(rewards), np.stack(dones)


def play_host(envs, actions):
    """The same over host env objects, reset when done (the frame after a done is the next episode's reset frame)."""
    cur = [e.reset() for e in envs]
    frames, rewards, dones = [np.stack(cur)], [], []
    for a in actions:
        r, d = np.zeros(len(envs), np.float32), np.zeros(len(envs), np.uint8)
        for i, e in enumerate(envs):
            cur[i], r[i], done, _ = e.step(int(a[i]))
            if done:
                d[i], cur[i] = 1, e.reset()
        frames.append(np.stack(cur))
        rewards.append(r)
        dones.append(d)
    return np.stack(frames), np.stack(rewards), np.stack(dones)


def paint(shape, bx, by, px, lx, ly, bricks):
    """The expected frame [1, H, W] of one written-out state: levels painted lowest first, so the later ones win (ball over paddle over
    trail over brick).  `bricks`: one string per brick row, '#' a brick, '.' none, column 0 first."""
    rows, cols, ch, cw, K, _ = shape
    f = np.zeros((1, rows * ch, cols * cw), np.uint8)

    def cell(r, c, v):
        f[0, r * ch:(r + 1) * ch, c * cw:(c + 1) * cw] = v

    assert len(bricks) == K and all(len(b) == cols for b in bricks)
    for k, b in enumerate(bricks):
        for c, ch_ in enumerate(b):
            if ch_ == '#':
                cell(k + 1, c, BRICK)
    cell(ly, lx, TRAIL)
    cell(rows - 1, px, PADDLE)
    cell(by, bx, BALL)
    return f


# Scripted episodes on the 4 x 3 grid with one brick row (bricks in row 1, the ball starts in row 2, the paddle in row 3 at column 1), every
# state written out by hand from the rules.  name -> (max_moves, the start codes of successive episodes,
#   [(action, reward, done, (bx, by, px, lx, ly, bricks)), ...]); the state after a move that ends the episode is the next episode's reset
# state.  Start code k: bx = k >> 1, d = 2 + (k & 1); d: 0 up-left, 1 up-right, 2 down-right, 3 down-left.
_SIDE = [
    (2, 0.0, 0, (2, 2, 2, 2, 2, ('###',))),  # code 4: (2,2) d2; paddle to 2; nx = 3 clamps to 2, d3; paddle row, bx == px: d0, ball stays in row 2
    (1, 1.0, 0, (1, 2, 2, 2, 2, ('#.#',))),  # d0 -> (1,1): a brick: removed, reward 1, ball keeps row 2, d3
]
_START0 = [
    (0, 0.0, 0, (1, 2, 0, 0, 2, ('###',))),  # code 0: (0,2) d2; paddle to 0; -> (1,3): bx == px: d1, ball (1,2)
    (2, 1.0, 0, (2, 2, 1, 1, 2, ('##.',))),  # d1 -> (2,1): brick, reward 1, d2
    (2, 0.0, 0, (2, 2, 2, 2, 2, ('##.',))),  # d2: nx = 3 clamps to 2, d3; paddle row, bx == px = 2: d0
]
SCRIPTS = {
    'side_bounce': (12, [4], _SIDE[:1]),
    'brick_hit': (12, [4], _SIDE),
    # d3 -> (0,3): bx = 1, nx = 0, paddle at 2: a miss; episode 2 (code 1: (0,2) d3, paddle 1): nx = -1 clamps to 0, d2; (0,3): bx = 0, nx = 0,
    # paddle 1: a miss again; episode 3 starts from code 0
    'miss': (12, [4, 1, 0], _SIDE + [(1, 0.0, 1, (0, 2, 1, 0, 2, ('###',))), (1, 0.0, 1, (0, 2, 1, 0, 2, ('###',)))]),
    'paddle_straight': (12, [0], _START0[:1]),
    'paddle_corner': (12, [0], [(1, 0.0, 0, (1, 2, 1, 0, 2, ('###',)))]),  # paddle stays at 1; -> (1,3): bx = 0 != px, nx == px: d0, ball (1,2)
    'top_bounce': (12, [1], [
        (0, 0.0, 0, (0, 2, 0, 0, 2, ('###',))),  # code 1: (0,2) d3; paddle to 0; nx = -1 clamps to 0, d2; paddle row, bx == px: d1
        (2, 1.0, 0, (1, 2, 1, 0, 2, ('#.#',))),  # d1 -> (1,1): brick, reward 1, d2
        (2, 0.0, 0, (2, 2, 2, 1, 2, ('#.#',))),  # d2 -> (2,3): bx = 1 != px = 2, nx == px: d0, ball (2,2)
        (0, 0.0, 0, (1, 1, 1, 2, 2, ('#.#',))),  # d0 -> (1,1): the brick is gone: nothing
        (0, 0.0, 0, (0, 0, 0, 1, 1, ('#.#',))),  # d0 -> (0,0)
        (0, 0.0, 0, (0, 0, 0, 0, 0, ('#.#',))),  # d0: nx = -1 clamps to 0, d1; ny = -1: ny = 0, d2: the ball stays, the trail joins it
    ]),
    'refill': (12, [0], _START0 + [
        (0, 1.0, 0, (1, 2, 1, 2, 2, ('#..',))),  # d0 -> (1,1): brick, reward 1, d3
        (1, 0.0, 0, (0, 2, 1, 1, 2, ('#..',))),  # d3 -> (0,3): bx == px = 1: d0, ball (0,2)
        (0, 1.0, 0, (0, 2, 0, 0, 2, ('...',))),  # d0: nx = -1 clamps to 0, d1; (0,1): the last brick, reward 1, d2
        (0, 0.0, 0, (1, 2, 0, 0, 2, ('###',))),  # d2 -> (1,3): no brick left: refill; bx == px = 0: d1, ball (1,2)
    ]),
    'cap': (3, [0, 0], _START0[:2] + [(2, 0.0, 1, (0, 2, 1, 0, 2, ('###',)))]),       # the third move bounces and is the cap: done, reward 0
    'cap_brick': (2, [0, 0], _START0[:1] + [(2, 1.0, 1, (0, 2, 1, 0, 2, ('###',)))]),  # the second move breaks a brick and is the cap
}
