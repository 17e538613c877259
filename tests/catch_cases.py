"""Cases for the device Catch env (MZ_ENV_CATCH, csrc/mz_catch.h): a numpy model of what the device does -- games.CatchEnv's rules for B envs
at once, plus the two things the host env leaves to its caller: the ball column's Philox draw and the staggered first episode -- the scripted
action sequences, and the shapes.  tests/test_catch_host.py holds the model to games.CatchEnv step for step (and shows that each planted
mistake is seen by a named case); tests/test_gpu_catch.py holds the device to host CatchEnv objects fed by `ball_col` / `first_row`."""
import numpy as np

from helpers import philox_uniforms

STREAM = 0x70000000  # the ball column's Philox stream (mz_catch.h CATCH_STREAM)

# name -> (rows, cols, cell_h, cell_w): the frame is [1, rows * cell_h, cols * cell_w]
SHAPES = {
    'c1': (12, 12, 1, 1),     # 12 x 12 frames, cells of one pixel
    'r6c4': (6, 4, 2, 3),     # 12 x 12 frames cut 6 x 4: cell width 3 (no multiple of 4), episodes of 5 moves
    'r5c5': (5, 5, 2, 3),     # 10 x 15 frames: 150 bytes (no multiple of 16 or of 4), so the renderer's 16-byte runs cross envs
    'wide': (12, 12, 1, 2),   # 12 x 24 frames, non-square cells
    'atari': (12, 12, 8, 8),  # 96 x 96, the Atari nets' frame
}
BUGS = ('paddle_after_catch', 'reward_sign', 'clip_off_by_one', 'col_prev_episode', 'stagger_every_episode', 'ball_in_paddle_row')
# the named case on which each planted mistake must show
SEEN_BY = {'paddle_after_catch': 'last_move', 'reward_sign': 'stay', 'clip_off_by_one': 'wall_right', 'col_prev_episode': 'stay',
           'stagger_every_episode': 'stay', 'ball_in_paddle_row': 'stay'}
SCRIPTS = ('stay', 'wall_left', 'wall_right', 'last_move', 'mixed')


def ball_col(seed, e, k, cols):
    """The ball column of env e, episode k."""
    u = philox_uniforms(seed, e, k, STREAM, 1)[0]
    return min(cols - 1, int(np.floor(u * cols)))


def first_row(e, rows):
    """The ball's row at the start of env e's episode 0 (later episodes: row 0)."""
    return e % (rows - 1)


class CatchModel:
    """B device Catch envs.  `bug` plants one mistake (BUGS)."""

    def __init__(self, B, rows, cols, cell_h, cell_w, seed, bug=None):
        assert bug is None or bug in BUGS
        self.B, self.rows, self.cols, self.ch, self.cw, self.seed, self.bug = B, rows, cols, cell_h, cell_w, seed, bug
        self.episode = np.zeros(B, np.int64)
        self.br = np.array([first_row(e, rows) for e in range(B)])
        self.bc = np.array([ball_col(seed, e, 0, cols) for e in range(B)])
        self.pc = np.full(B, cols // 2)

    def frames(self):
        """uint8 [B, 1, H, W]: what the next act sees."""
        out = np.zeros((self.B, 1, self.rows * self.ch, self.cols * self.cw), np.uint8)
        for e in range(self.B):
            r, c, p = int(self.br[e]), int(self.bc[e]), int(self.pc[e])
            out[e, 0, r * self.ch:(r + 1) * self.ch, c * self.cw:(c + 1) * self.cw] = 255
            out[e, 0, (self.rows - 1) * self.ch:, p * self.cw:(p + 1) * self.cw] = 255
        return out

    def step(self, actions):
        """-> (reward float32 [B], done uint8 [B]); a finished env is at its next episode's reset state afterwards."""
        reward, done = np.zeros(self.B, np.float32), np.zeros(self.B, np.uint8)
        last = self.rows if self.bug == 'ball_in_paddle_row' else self.rows - 1
        for e in range(self.B):
            old = int(self.pc[e])
            hi = self.cols if self.bug == 'clip_off_by_one' else self.cols - 1
            self.pc[e] = min(max(old + int(actions[e]) - 1, 0), hi)
            self.br[e] += 1
            if self.br[e] != last:
                continue
            caught = self.bc[e] == (old if self.bug == 'paddle_after_catch' else self.pc[e])
            reward[e] = (1.0 if caught else -1.0) * (-1.0 if self.bug == 'reward_sign' else 1.0)
            done[e] = 1
            self.episode[e] += 1
            k = int(self.episode[e]) - (1 if self.bug == 'col_prev_episode' else 0)
            self.br[e] = first_row(e, self.rows) if self.bug == 'stagger_every_episode' else 0
            self.bc[e] = ball_col(self.seed, e, k, self.cols)
            self.pc[e] = self.cols // 2
        return reward, done


def host_envs(B, rows, cols, cell_h, cell_w, seed, episodes=64):
    """B games.CatchEnv objects that play what the device plays: the regenerated ball columns and the stagger."""
    from muzero_amd.games import CatchEnv

    return [CatchEnv(rows, cols, cell_h, cell_w, ball_cols=[ball_col(seed, e, k, cols) for k in range(episodes)], first_row=first_row(e, rows))
            for e in range(B)]


def script(name, B, rows, cols, seed, moves):
    """int32 [moves, B]: the scripted actions of a named case.  'last_move' stays until an episode's last move and then steps towards the
    ball (a catch exactly where the ball starts one column off); 'mixed' is a fixed pseudo-random sequence."""
    if name in ('stay', 'wall_left', 'wall_right'):
        return np.full((moves, B), {'stay': 1, 'wall_left': 0, 'wall_right': 2}[name], np.int32)
    if name == 'mixed':
        return np.random.RandomState(1234).randint(0, 3, size=(moves, B)).astype(np.int32)
    assert name == 'last_move'
    m = CatchModel(B, rows, cols, 1, 1, seed)
    out = np.ones((moves, B), np.int32)
    for t in range(moves):
        final = m.br == rows - 2
        out[t] = np.where(final, 1 + np.sign(m.bc - m.pc), 1)
        m.step(out[t])
    return out


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
