"""Cases for the image arena (mz_arena_reset_catch / mz_arena_reset_external, csrc/mz_arena_image.h): a numpy model of what the device does
for B Catch games in lock-step -- games.CatchEnv's rules, StackFrameAndAction's roots, and what the arena adds: no restart, a finished
env frozen with its history, root and record, the tally.  tests/test_arena_image_host.py holds the model to games.make_catch_env objects
byte for byte (and shows that each planted mistake is seen by a named case); tests/test_gpu_arena_image.py holds the device to the same
host objects."""
import numpy as np

import catch_cases as cc

SHAPES = cc.SHAPES
STACKS = (2, 4)
BUGS = ('frozen_history_advances', 'first_action_plane', 'first_frame_not_replicated', 'freeze_late', 'reward_after_freeze', 'totals_count_frozen')
# the named case (shape, S, script) on which each planted mistake must show
SEEN_BY = {'frozen_history_advances': ('r6c4', 2, 'mixed'), 'first_action_plane': ('c1', 2, 'stay'), 'first_frame_not_replicated': ('c1', 4, 'stay'),
           'freeze_late': ('r6c4', 2, 'stay'), 'reward_after_freeze': ('r6c4', 4, 'wall_left'), 'totals_count_frozen': ('wide', 2, 'stay')}
SCRIPTS = ('stay', 'wall_left', 'mixed')
NUM_ACTIONS = 3


def layout(B, rows, cols):
    """Ball columns and start rows of a batch: every column in turn, start rows staggered over 0 .. rows - 2 (both ends in one batch)."""
    assert B >= rows - 1
    return np.arange(B) % cols, np.arange(B) % (rows - 1)


def script(name, B, plies):
    if name in ('stay', 'wall_left'):
        return np.full((plies, B), {'stay': 1, 'wall_left': 0}[name], np.int32)
    assert name == 'mixed'
    return np.random.RandomState(4321).randint(0, 3, size=(plies, B)).astype(np.int32)


def action_value(a):
    """float32 of the reference's (action + 1) / num_actions (a Python float)."""
    return np.float32((a + 1) / NUM_ACTIONS)


class ImageArenaModel:
    """B Catch games of the image arena.  `bug` plants one mistake (BUGS)."""

    def __init__(self, rows, cols, cell_h, cell_w, S, ball_cols, start_rows, bug=None):
        assert bug is None or bug in BUGS
        self.rows, self.cols, self.ch, self.cw, self.S, self.bug = rows, cols, cell_h, cell_w, S, bug
        self.B = B = len(ball_cols)
        self.br, self.bc, self.pc = np.array(start_rows).copy(), np.array(ball_cols).copy(), np.full(B, cols // 2)
        self.live = np.ones(B, bool)
        self.late = np.zeros(B, bool)  # ('freeze_late': done, but still played for one ply)
        self.length = np.zeros(B, np.int64)
        self.ret = np.zeros(B, np.float64)
        self.last_reward = np.zeros(B, np.float32)
        self.draws = self.finished_plies = 0
        self.hist = [None] * B      # per env: S uint8 frames, newest first
        self.hist_act = [None] * B  # per env: S actions, newest first
        self.prev = np.zeros(B, np.int64)
        self.ply = 0
        self._root = np.zeros((B, 2 * S, rows * cell_h, cols * cell_w), np.float32)

    def frame(self, e):
        f = np.zeros((self.rows * self.ch, self.cols * self.cw), np.uint8)
        r, c, p = int(self.br[e]), int(self.bc[e]), int(self.pc[e])
        f[r * self.ch:(r + 1) * self.ch, c * self.cw:(c + 1) * self.cw] = 255
        f[(self.rows - 1) * self.ch:, p * self.cw:(p + 1) * self.cw] = 255
        return f

    def roots(self):
        """float32 [B, 2 S, H, W]: this ply's roots.  Builds the live envs' (and files their newest frame); a frozen env keeps its own."""
        S = self.S
        for e in range(self.B):
            if not self.live[e] and self.bug != 'frozen_history_advances':
                continue
            f = self.frame(e)
            if self.ply == 0:
                self.hist[e] = [f] + [np.zeros_like(f) if self.bug == 'first_frame_not_replicated' else f] * (S - 1)
                self.hist_act[e] = [1 if self.bug == 'first_action_plane' else 0] * S
            else:
                self.hist[e] = [f] + self.hist[e][:-1]
                self.hist_act[e] = [int(self.prev[e])] + self.hist_act[e][:-1]
            for k in range(S):
                self._root[e, k] = self.hist[e][k].astype(np.float32) / np.float32(255.0)
                self._root[e, S + k] = action_value(self.hist_act[e][k])
        return self._root.copy()

    def step(self, actions):
        """One ply: the live envs move."""
        for e in range(self.B):
            if not self.live[e]:
                if self.bug == 'reward_after_freeze':
                    self.ret[e] += float(self.last_reward[e])
                if self.bug == 'totals_count_frozen':
                    self.finished_plies += 1
                continue
            a = int(actions[e])
            self.prev[e] = a
            self.length[e] += 1
            if self.late[e]:  # the ply a late freeze plays on: the ball rests in the last row
                self.live[e] = False
                self.draws += 1
                self.finished_plies += int(self.length[e])
                continue
            pc = min(max(int(self.pc[e]) + a - 1, 0), self.cols - 1)
            br = int(self.br[e]) + 1
            done = br == self.rows - 1
            r = np.float32((1.0 if self.bc[e] == pc else -1.0) if done else 0.0)
            self.ret[e] += float(r)
            self.last_reward[e] = r
            if done and self.bug == 'freeze_late':
                self.late[e] = True
            elif done:
                self.live[e] = False
                self.draws += 1
                self.finished_plies += int(self.length[e])
            else:
                self.br[e], self.pc[e] = br, pc
        self.ply += 1


def play_model(model, actions):
    """-> dict of per-ply arrays: root [T, B, ...], live [T, B] (when the ply began), length / ret [T, B] and draws / finished_plies / n_live
    [T] after it."""
    out = dict(root=[], live=[], length=[], ret=[], draws=[], finished_plies=[], n_live=[])
    for a in actions:
        out['live'].append(model.live.copy())
        out['root'].append(model.roots())
        model.step(a)
        out['length'].append(model.length.copy())
        out['ret'].append(model.ret.copy())
        out['draws'].append(model.draws)
        out['finished_plies'].append(model.finished_plies)
        out['n_live'].append(int(model.live.sum()))
    return {k: np.array(v) for k, v in out.items()}


def host_envs(rows, cols, cell_h, cell_w, S, ball_cols, start_rows):
    """games.make_catch_env objects that start where the arena's envs start."""
    from muzero_amd.games import make_catch_env

    return [make_catch_env(rows, cols, cell_h, cell_w, stack_history=S, start_row=int(r), ball_cols=[int(c)]) for c, r in zip(ball_cols, start_rows)]


def play_host(envs, actions):
    """The same over host env objects, each played once to its end and then left alone: a finished env keeps the last root it moved on."""
    B = len(envs)
    obs = [np.asarray(e.reset(), np.float32) for e in envs]
    live = np.ones(B, bool)
    length, ret = np.zeros(B, np.int64), np.zeros(B, np.float64)
    draws = plies = 0
    out = dict(root=[], live=[], length=[], ret=[], draws=[], finished_plies=[], n_live=[])
    for a in actions:
        out['live'].append(live.copy())
        out['root'].append(np.stack(obs))
        for i, e in enumerate(envs):
            if not live[i]:
                continue
            nxt, r, d, _ = e.step(int(a[i]))
            length[i] += 1
            ret[i] += float(np.float32(r))
            if d:
                live[i] = False
                draws += 1
                plies += int(length[i])
            else:
                obs[i] = np.asarray(nxt, np.float32)
        out['length'].append(length.copy())
        out['ret'].append(ret.copy())
        out['draws'].append(draws)
        out['finished_plies'].append(plies)
        out['n_live'].append(int(live.sum()))
    return {k: np.array(v) for k, v in out.items()}
