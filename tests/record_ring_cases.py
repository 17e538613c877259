"""The window rule of the compact record ring (include/mzplanner.h, MZ_RECORD_FRAMES_U8) as a numpy function, the scripted uint8 frame
env it is checked on, and three wrong rules a test must be able to tell from it.  No GPU, no torch: tests/test_record_ring_host.py holds
the rule to `games.StackFrameAndAction(games.ScaledFloatFrame(env), S, True)` + `replay.encode_state`, tests/test_gpu_record_ring.py
holds the kernels to the float32 record ring.

A record ring of host-stepped envs keeps, per env and move m, the uint8 frame the host uploaded for act m, the action the search chose
and the done flag.  With first(m) = the largest m' <= m that starts an episode (m' == 0 or done[m' - 1]), the observation of move m is
  frame block k (0 = newest, k < S) = frames[max(m - k, first(m))]
  action k                          = actions[m - k - 1] if m - k > first(m) else 0
and its frames_u8 replay row is those S frames' bytes in that order, the S action bytes, zero padding to a multiple of 16.
"""
import functools
import types

import numpy as np

# name -> (C, H, W, S, A): a frame of 9 bytes (no multiple of 16), C > 1, 256 actions, a deeper stack, the 16-byte frame
GEOMETRIES = {
    'odd9': (1, 3, 3, 2, 3),
    'c3': (3, 4, 4, 2, 4),
    'a256': (1, 4, 4, 4, 256),
    'deep': (2, 2, 4, 5, 6),
    'f16': (1, 4, 4, 3, 5),
}
# episode lengths, cycled: length 1 twice in a row, lengths below every S above, and long ones whose windows are full
LENGTHS = (1, 1, 2, 7, 3, 1, 4, 9, 2, 6)
MOVES = 60
SEEDS = tuple(range(4))


@functools.lru_cache(maxsize=None)
def script(name, seed):
    """What one env's host loop sees over MOVES moves: frames[m] (the frame uploaded for act m; one more than MOVES, for the reset after
    the last move), actions[m] (adjacent ones differ, so a shifted action index shows), done[m]."""
    C, H, W, S, A = GEOMETRIES[name]
    rs = np.random.RandomState(1000 * seed + sum(map(ord, name)))
    frames = rs.randint(0, 256, size=(MOVES + 1, C, H, W)).astype(np.uint8)
    actions = np.empty(MOVES, np.int64)
    actions[0] = rs.randint(A)
    for m in range(1, MOVES):
        actions[m] = (actions[m - 1] + 1 + rs.randint(A - 1)) % A
    done, m, j = np.zeros(MOVES, np.uint8), 0, seed
    while True:
        m += LENGTHS[j % len(LENGTHS)]
        j += 1
        if m > MOVES:
            break
        done[m - 1] = 1
    for a in (frames, actions, done):
        a.setflags(write=False)
    return types.SimpleNamespace(name=name, C=C, H=H, W=W, S=S, A=A, frames=frames, actions=actions, done=done, frame_spec=(S, C, H, W, A))


class ScriptedFrames:
    """A uint8 image env that plays `frames` and `done` back: reset() and step() hand out frames[i] for the i-th act of the run (what a
    done step itself returns is dropped by every actor loop, so it is zeros); rewards are small integers by move."""

    def __init__(self, frames, done, num_actions):
        self.frames, self.done, self.num_actions = frames, done, int(num_actions)
        self.observation_shape = tuple(frames.shape[1:])
        self.i = 0
        self.taken = []

    def reset(self):
        return self.frames[self.i].copy()

    def step(self, action):
        self.taken.append(int(action))
        d = bool(self.done[self.i])
        r = float(self.i % 5 - 2)
        self.i += 1
        return (np.zeros_like(self.frames[0]) if d else self.frames[self.i].copy()), r, d, {}


def first_of(done, m):
    while m > 0 and not done[m - 1]:
        m -= 1
    return m


def window_row(sc, m, rule='window'):
    """The frames_u8 replay row of move m from the records of `sc` (frames, actions, done).  `rule`: 'window' is the rule; the others are
    the mistakes a test must catch -- 'no_first' clamps the history at the start of the run instead of the episode, 'action_shift' takes
    action k from actions[m - k], 'plane_order' writes the planes channel-major (c * S + k)."""
    S, C, HW, A = sc.S, sc.C, sc.H * sc.W, sc.A
    first = 0 if rule == 'no_first' else first_of(sc.done, m)
    P = S * C * HW
    row = np.zeros((P + S + 15) // 16 * 16, np.uint8)
    blocks = np.stack([sc.frames[max(m - k, first)].reshape(C, HW) for k in range(S)])  # [S][C][HW]
    row[:P] = (blocks.transpose(1, 0, 2) if rule == 'plane_order' else blocks).reshape(-1)
    for k in range(S):
        if m - k > first:
            row[P + k] = sc.actions[m - k if rule == 'action_shift' else m - k - 1]
    return row


def window_rows(sc, rule='window'):
    return np.stack([window_row(sc, m, rule) for m in range(MOVES)])


@functools.lru_cache(maxsize=None)
def stacker_observations(name, seed):
    """The float32 observations [MOVES, S * (C + 1), H, W] the project's wrappers show an actor over the script."""
    from muzero_amd import games

    sc = script(name, seed)
    env = games.StackFrameAndAction(games.ScaledFloatFrame(ScriptedFrames(sc.frames, sc.done, sc.A)), sc.S, True)
    out, obs = [], env.reset()
    for m in range(MOVES):
        out.append(np.asarray(obs, np.float32))
        obs, _, d, _ = env.step(int(sc.actions[m]))
        if d:
            obs = env.reset()
    out = np.stack(out)
    out.setflags(write=False)
    return out
