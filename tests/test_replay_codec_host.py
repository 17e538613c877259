"""The compact state formats of the replay ('int8', 'frames_u8'; muzero_amd/replay.py encode_state / decode_state), proved on the host (no
GPU): the codec is exact for every value the producers emit, refuses everything else naming the element, and a compact host replay is
draw for draw the float32 one."""
import itertools

import numpy as np
import pytest
import torch

from muzero_amd import games
from muzero_amd import replay as rp
from muzero_amd.replay import PrioritizedReplay, Transition, decode_state, encode_state

A_SET, S_SET, C_SET = (2, 3, 6, 18, 256), (1, 4, 8), (1, 3)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frames_obs(rng, n, S, C, H, W, A):
    """n observations the way StackFrameAndAction + ScaledFloatFrame build them, from random bytes and actions"""
    b = rng.randint(0, 256, size=(n, S * C, H, W)).astype(np.uint8)
    a = rng.randint(0, A, size=(n, S))
    planes = ((a + 1) / A).astype(np.float32)[:, :, None, None] * np.ones((1, 1, H, W), np.float32)
    return np.concatenate([b.astype(np.float32) / 255.0, planes], axis=1), b, a


@pytest.mark.parametrize('A,S,C', list(itertools.product(A_SET, S_SET, C_SET)))
def test_round_trip_is_bit_exact_for_every_byte_and_every_action(A, S, C):
    for H, W in ((3, 3), (5, 5), (4, 4)):
        P = S * C * H * W
        row_bytes = (P + S + 15) // 16 * 16
        assert rp.state_row_bytes('frames_u8', (S * (C + 1), H, W), (S, C, H, W, A)) == row_bytes
        n = max(-(-256 // P), -(-A // S)) + 1
        # every byte value and every action at least once, in the scalar expressions the device uses
        b = (np.arange(n * P) % 256).astype(np.uint8).reshape(n, S * C, H, W)
        a = (np.arange(n * S) % A).reshape(n, S)
        assert set(b.ravel()) == set(range(256)) and set(a.ravel()) == set(range(A))
        x = np.empty((n, S * (C + 1), H, W), np.float32)
        x[:, :S * C] = b.astype(np.float32) / np.float32(255.0)
        for i, k in itertools.product(range(n), range(S)):
            x[i, S * C + k] = np.float32((float(a[i, k]) + 1.0) / float(A))
        rows = encode_state(x, 'frames_u8', (S, C, H, W, A))
        assert rows.dtype == np.uint8 and rows.shape == (n, row_bytes)
        assert (rows[:, :P] == b.reshape(n, P)).all() and (rows[:, P:P + S] == a).all() and (rows[:, P + S:] == 0).all()
        back = decode_state(rows, 'frames_u8', (S, C, H, W, A))
        assert back.dtype == np.float32 and back.shape == x.shape and (bits(back) == bits(x)).all()
        one = encode_state(x[0], 'frames_u8', (S, C, H, W, A))  # a single observation: no leading axis
        assert one.shape == (row_bytes,) and (one == rows[0]).all()


def test_row_sizes_of_the_issue():
    assert rp.state_row_bytes('frames_u8', (8, 96, 96), (4, 1, 96, 96, 18)) == 36880
    assert rp.state_row_bytes('int8', (9, 15, 15)) == 2025 and rp.state_row_bytes('f32', (8, 96, 96)) == 294912
    # 3 x 3 and 5 x 5: the plane size is no multiple of 4 and the row no multiple of 16 before padding
    assert (2 * 1 * 9 + 2) % 16 and (2 * 1 * 25 + 2) % 16


class ScriptedEnv:
    """uint8 frames [C, H, W] from a fixed stream; episodes of `length` steps"""

    def __init__(self, C, H, W, A, length, seed):
        self.observation_shape, self.num_actions, self.length = (C, H, W), A, length
        self.rng = np.random.RandomState(seed)
        self.t = 0

    def _frame(self):
        return self.rng.randint(0, 256, size=self.observation_shape).astype(np.uint8)

    def reset(self):
        self.t = 0
        return self._frame()

    def step(self, action):
        self.t += 1
        return self._frame(), 1.0, self.t >= self.length, {}


@pytest.mark.parametrize('S,C,H,W,A', [(2, 1, 3, 3, 3), (4, 1, 5, 5, 18), (8, 3, 4, 4, 6), (1, 3, 5, 5, 2)])
def test_decoded_rows_are_the_wrappers_observations_across_a_reset(S, C, H, W, A):
    env = games.StackFrameAndAction(games.ScaledFloatFrame(ScriptedEnv(C, H, W, A, 5, 3)), S, True)
    acts = np.random.RandomState(1).randint(0, A, size=64)
    seen, obs = [], env.reset()
    for t in range(13):  # two resets inside
        seen.append(obs)
        obs, _, done, _ = env.step(int(acts[t]))
        if done:
            seen.append(obs)
            obs = env.reset()
    x = np.stack(seen)
    assert x.dtype == np.float32 and x.shape[1:] == (S * (C + 1), H, W)
    rows = encode_state(x, 'frames_u8', (S, C, H, W, A))
    assert (bits(decode_state(rows, 'frames_u8', (S, C, H, W, A))) == bits(x)).all()
    assert (rows[0, S * C * H * W:S * C * H * W + S] == 0).all()  # after a reset every action byte is action 0


def test_refusals_name_the_element():
    S, C, H, W, A = 2, 1, 3, 3, 6
    spec = (S, C, H, W, A)
    x, _, _ = frames_obs(np.random.RandomState(0), 3, *spec)
    encode_state(x, 'frames_u8', spec)
    y = x.copy()
    y[1, 1, 2, 0] = np.nextafter(np.float32(77.0) / np.float32(255.0), np.float32(1.0))  # one ulp off b / 255
    with pytest.raises(ValueError, match=r'item 1, plane 1, pixel 6'):
        encode_state(y, 'frames_u8', spec)
    y = x.copy()
    y[2, S * C + 1, 1, 1] = np.float32(1.0 / 6.0) if bits(y[2, S * C + 1, 0, 0]) != bits(np.float32(1.0 / 6.0)) else np.float32(2.0 / 6.0)
    with pytest.raises(ValueError, match=r'item 2, plane 3, pixel 4\).*constant'):
        encode_state(y, 'frames_u8', spec)
    y = x.copy()
    y[0, S * C] = np.float32(0.5 / 6.0)  # a constant plane, but of no action
    with pytest.raises(ValueError, match=r'item 0, plane 2, pixel 0\).*not \(a \+ 1\) / 6'):
        encode_state(y, 'frames_u8', spec)
    y = x.copy()
    y[0, S * C] = np.float32(7.0 / 6.0)  # action 6 of 6
    with pytest.raises(ValueError, match=r'item 0, plane 2, pixel 0'):
        encode_state(y, 'frames_u8', spec)
    with pytest.raises(ValueError, match=r'A = 257'):
        encode_state(x, 'frames_u8', (S, C, H, W, 257))
    with pytest.raises(ValueError, match=r'A = 257'):
        PrioritizedReplay(4, 0.0, 0.0, np.random.RandomState(0), state_format='frames_u8', frame_spec=(S, C, H, W, 257))
    with pytest.raises(ValueError, match='frame_spec'):
        encode_state(x, 'frames_u8', (S, C, H, 4, A))
    board = np.zeros((9, 3, 3), np.float32)
    board[4, 1, 2] = 0.5
    with pytest.raises(ValueError, match=r'element \(4, 1, 2\) = .*0\.5'):
        encode_state(board, 'int8')
    for v in (128.0, -129.0, np.nan, -0.0, 1e-40):
        board[4, 1, 2] = v
        with pytest.raises(ValueError, match=r'element \(4, 1, 2\)'):
            encode_state(board, 'int8')
    board[4, 1, 2] = -128.0
    board[0, 0, 0] = 127.0
    assert (bits(decode_state(encode_state(board, 'int8'), 'int8')) == bits(board)).all()
    with pytest.raises(ValueError, match='state_dtype'):
        PrioritizedReplay(4, 0.0, 0.0, np.random.RandomState(0), state_format='int8', state_dtype=torch.uint8)
    with pytest.raises(ValueError, match='state_format'):
        PrioritizedReplay(4, 0.0, 0.0, np.random.RandomState(0), state_format='u8')


def _items(fmt, n, K=3):
    rng = np.random.RandomState(11)
    if fmt == 'int8':
        states, A = (rng.uniform(size=(n, 9, 3, 3)) < 0.4).astype(np.float32), 10
    else:
        states, A = frames_obs(rng, n, 2, 1, 5, 5, 6)[0], 6
    return [Transition(states[i], rng.randint(0, A, size=K).astype(np.int8), rng.dirichlet(np.ones(A), size=K).astype(np.float32),
                       rng.normal(size=K).astype(np.float32), rng.normal(size=K).astype(np.float32)) for i in range(n)]


@pytest.mark.parametrize('fmt,spec', [('int8', None), ('frames_u8', (2, 1, 5, 5, 6))])
@pytest.mark.parametrize('alpha', [0.0, 0.6])
def test_compact_replay_is_the_float32_replay_draw_for_draw(fmt, spec, alpha):
    cap, items = 7, _items(fmt, 19)
    f32 = PrioritizedReplay(cap, alpha, 0.4, np.random.RandomState(5))
    cmp_ = PrioritizedReplay(cap, alpha, 0.4, np.random.RandomState(5), state_format=fmt, frame_spec=spec)

    def same_draw(batch):
        np.random.seed(99)  # (proportional replay draws from the process-global stream, as upstream)
        a = f32.sample(batch)
        np.random.seed(99)
        b = cmp_.sample(batch)
        assert (a[1] == b[1]).all() and (bits(a[2]) == bits(b[2])).all()
        assert b[0].state.dtype == np.float32 and b[0].state.shape == a[0].state.shape and (bits(a[0].state) == bits(b[0].state)).all()
        for f in ('action', 'pi_prob', 'value', 'reward'):
            assert np.array_equal(getattr(a[0], f), getattr(b[0], f))
        np.random.seed(98)
        ta = f32.sample_tensors(batch)
        np.random.seed(98)
        tb = cmp_.sample_tensors(batch)
        assert (ta[1] == tb[1]).all() and tb[0].state.dtype == torch.float32 and torch.equal(ta[0].state.view(torch.int32), tb[0].state.view(torch.int32))
        return a[1]

    for i, it in enumerate(items[:5]):
        f32.add(it, 0.5 + i)
        cmp_.add(it, 0.5 + i)
    same_draw(4)
    for lo in (5, 12):  # two batches of `cap` items: the ring wraps twice
        rest = Transition(*[np.stack([getattr(it, f) for it in items[lo:lo + 7]]) for f in Transition._fields])
        pr = np.linspace(0.1, 3.0, 7) + lo
        f32.add_batch(rest, pr)
        cmp_.add_batch(rest, pr)
    assert cmp_.num_added == f32.num_added == 19 and cmp_.size == cap
    picks = same_draw(6)
    f32.update_priorities(picks[:5], np.arange(5) + 0.25)
    cmp_.update_priorities(picks[:5], np.arange(5) + 0.25)
    same_draw(7)
    for a, b in zip(f32.get(range(cap)), cmp_.get(range(cap))):
        assert b.state.dtype == np.float32 and b.state.shape == a.state.shape and (bits(a.state) == bits(b.state)).all()
    with pytest.raises(ValueError):  # what the format cannot hold is refused at the add, naming the element
        cmp_.add(items[0]._replace(state=items[0].state + np.float32(0.25)), 1.0)
    assert cmp_.num_added == 19


def test_storage_is_capacity_times_row_bytes_and_the_size_check_counts_it():
    spec = (4, 1, 96, 96, 18)
    r = PrioritizedReplay(3, 0.0, 0.0, np.random.RandomState(0), state_format='frames_u8', frame_spec=spec)
    r.allocate(dict(state=(8, 96, 96), action=(5,), pi_prob=(5, 18), value=(5,), reward=(5,)))
    st = r._ring['state']
    assert st.dtype == torch.uint8 and tuple(st.shape) == (3, 36880) and st.numel() * st.element_size() == 3 * 36880
    assert r._ring.state_format == 'frames_u8' and r._ring.frame_spec == spec
    b = PrioritizedReplay(5, 0.0, 0.0, np.random.RandomState(0), state_format='int8')
    b.allocate(dict(state=(9, 15, 15), action=(5,), pi_prob=(5, 226), value=(5,), reward=(5,)))
    assert b._ring['state'].dtype == torch.int8 and b._ring['state'].numel() == 5 * 2025
    with pytest.raises(ValueError, match='frame_spec'):
        PrioritizedReplay(3, 0.0, 0.0, np.random.RandomState(0), state_format='frames_u8', frame_spec=spec).allocate(
            dict(state=(8, 84, 84), action=(5,), pi_prob=(5, 18), value=(5,), reward=(5,)))
    # the size check: a capacity whose compact rows fit where the float32 rows cannot, and one that fits neither
    import os

    phys = os.sysconf('SC_PHYS_PAGES') * os.sysconf('SC_PAGE_SIZE')
    other = 5 + 4 * (5 * 18 + 5 + 5)
    cap_mid = int(phys / (294912 + other)) * 2  # float32: about twice the machine; frames_u8: a quarter of it
    shapes = dict(state=(8, 96, 96), action=(5,), pi_prob=(5, 18), value=(5,), reward=(5,))
    with pytest.raises(MemoryError):
        PrioritizedReplay(cap_mid, 0.0, 0.0, np.random.RandomState(0)).allocate(shapes)
    big = PrioritizedReplay(cap_mid, 0.0, 0.0, np.random.RandomState(0), state_format='frames_u8', frame_spec=spec)
    big.allocate(shapes)  # (zero pages: committed lazily)
    assert tuple(big._ring['state'].shape) == (cap_mid, 36880)
    del big
    with pytest.raises(MemoryError):
        PrioritizedReplay(int(phys / (36880 + other)) * 2, 0.0, 0.0, np.random.RandomState(0), state_format='frames_u8', frame_spec=spec).allocate(shapes)


@pytest.mark.parametrize('fmt,spec', [('int8', None), ('frames_u8', (2, 1, 5, 5, 6))])
def test_get_state_set_state_round_trip(fmt, spec):
    items = _items(fmt, 6)
    a = PrioritizedReplay(4, 0.0, 0.0, np.random.RandomState(2), state_format=fmt, frame_spec=spec)
    for i, it in enumerate(items):
        a.add(it, 1.0 + i)
    saved = a.get_state()
    assert saved['state_format'] == fmt and saved['frame_spec'] == spec
    b = PrioritizedReplay(4, 0.0, 0.0, np.random.RandomState(2), state_format=fmt, frame_spec=spec)
    b.set_state(saved)
    assert b.num_added == 6 and b._ring.state_format == fmt
    for x, y in zip(a.get(range(4)), b.get(range(4))):
        assert (bits(x.state) == bits(y.state)).all() and np.array_equal(x.action, y.action)
    assert (bits(a.sample(4)[0].state) == bits(b.sample(4)[0].state)).all()
    with pytest.raises(ValueError, match='state_format|stores states'):
        PrioritizedReplay(4, 0.0, 0.0, np.random.RandomState(2)).set_state(saved)
    assert 'state_format' not in PrioritizedReplay(4, 0.0, 0.0, np.random.RandomState(2)).get_state()
