"""Compact replay states on the device ('int8', 'frames_u8'): the planner's k_epi_states writes them, the conv learner's k_lc_gather reads
them, and both are EXACT -- two planners with one seed, one writing a float32 ring and one a compact ring, stay equal move for move
(count, every other field byte for byte, decode_state(compact row) == float32 row bit for bit, zero padding) through ring wraps, moves
that emit more items than the ring holds and a flush that meets an episode end; the learner's gradient, loss, priorities and weights
over the two rings are the same bytes; what a format cannot hold is refused by name; and the float32 ring is still the host
EpisodeAssembler's."""
import functools
import types

import numpy as np
import pytest
import torch

from helpers import build_conv, build_mlp, mlp_case

pytestmark = pytest.mark.gpu

FIELDS = ('action', 'pi_prob', 'value', 'reward')
# acc_seq_length + unroll_steps + td_steps = 7: an episode of exactly 7 moves flushes and ends on the same move (7 items at once)
CFG = types.SimpleNamespace(is_board_game=False, acc_seq_length=3, unroll_steps=2, td_steps=2, discount=0.997)
BOARD_CFG = types.SimpleNamespace(is_board_game=True, acc_seq_length=3, unroll_steps=2, td_steps=2, discount=1.0)
LENS = (7, 2, 9, 4, 7, 3, 11, 5)  # staggered episode lengths: env e's j-th episode lasts LENS[(e + 3 j) % 8] moves

# name -> (net builder, frame shape or None, S, actions, envs, ring capacity, moves, simulations, device env)
RUNS = {
    'mlp44': (lambda: build_mlp(('f44', (4, 4, 4), 3, 32, 7, 5, 16, 41)), (1, 4, 4), 2, 3, 8, 5, 26, 4, None),
    'mlp33': (lambda: build_mlp(('f33', (4, 3, 3), 3, 32, 7, 5, 16, 42)), (1, 3, 3), 2, 3, 8, 5, 26, 4, None),
    'atari': (lambda: build_conv(('atari_s8', 'atari', (8, 96, 96), 6, 1, 8, 11, 11, 24)), (1, 96, 96), 4, 6, 4, 6, 16, 3, None),
    'ttt': (lambda: build_conv(('board3', 'board', (9, 3, 3), 10, 2, 16, 1, 1, 21)), None, 0, 10, 8, 7, 24, 4, 'ENV_TICTACTOE'),
    'gomoku5': (lambda: build_conv(('board5g', 'board', (9, 5, 5), 26, 1, 8, 1, 1, 22)), None, 0, 26, 8, 8, 40, 2, 'ENV_GOMOKU'),
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _snapshot(rp, origin):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in rp._ring.items()}, rp._attached[0].cpu().numpy().copy(), origin.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def run(name):
    """Both planners of a case, stepped in lock-step; everything the tests below read, computed once."""
    from muzero_amd import planner as pl
    from muzero_amd.pipeline import EpisodeAssembler
    from muzero_amd.replay import PrioritizedReplay

    make, fshape, S, A, B, cap, moves, sims, dev_env = RUNS[name]
    net = make()
    spec = net.planner_spec()
    shape = tuple(spec['input_shape'])
    board = dev_env is not None
    cfg = BOARD_CFG if board else CFG
    fmt = 'int8' if board else 'frames_u8'
    frame_spec = None if board else (S,) + fshape + (A,)
    kw = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0)) if board else dict(discount=0.997)
    side = {}
    for which in ('f32', fmt):
        p = pl.Planner(pl.make_mz_config(spec, None, num_envs=B, seed=5, num_simulations=sims, **kw), 0)
        p.load_state_dict(net.state_dict())
        rp = PrioritizedReplay(cap, 0.0, 0.0, np.random.RandomState(0), device='cuda', **(dict(state_format=fmt, frame_spec=frame_spec) if which != 'f32' else {}))
        origin = p.attach_replay(rp, cfg, obs_shape=shape, with_origin=True)
        if board:
            p.selfplay_reset(getattr(pl, dev_env))
        else:
            p.selfplay_reset_external(stack_history=S, is_obs_image=True, frame_shape=fshape, frame_u8=True)
        side[which] = (p, rp, origin)
    rs = np.random.RandomState(77)
    left, episode = [LENS[e % 8] for e in range(B)], [0] * B
    asm, host, counts = [EpisodeAssembler(cfg, 1, shape) for _ in range(B)], [[] for _ in range(B)], []
    for m in range(moves):
        if board:
            for p, _, _ in side.values():
                p.selfplay_step(-1.0, 1)
        else:
            frames = rs.randint(0, 256, size=(B,) + fshape).astype(np.uint8)
            rew = rs.randint(-2, 3, size=B).astype(np.float32)
            done = np.zeros(B, np.uint8)
            for e in range(B):
                left[e] -= 1
                if left[e] == 0:
                    done[e], episode[e] = 1, episode[e] + 1
                    left[e] = LENS[(e + 3 * episode[e]) % 8]
            acts = [p.external_act(frames, np.ones((B, A), np.uint8), 1, 1, 1.0) for p, _, _ in side.values()]
            assert np.array_equal(acts[0], acts[1])
            for p, _, _ in side.values():
                p.external_commit(rew, done)
        for p, _, _ in side.values():
            p.synchronize()  # (a move's epilogue is only enqueued when the call returns)
        counts.append(tuple(rp.num_added for _, rp, _ in side.values()))
        rec = side['f32'][0].selfplay_read(1)
        for b in range(B):
            host[b].extend(asm[b].feed({k: v[:, b:b + 1] for k, v in rec.items()}))
    snap = {which: _snapshot(rp, origin) for which, (_, rp, origin) in side.items()}
    return types.SimpleNamespace(name=name, net=net, fmt=fmt, frame_spec=frame_spec, shape=shape, B=B, cap=cap, A=A, side=side, counts=counts, host=host,
                                 snap=snap, n=counts[-1][0])


@pytest.mark.parametrize('name', list(RUNS))
def test_compact_ring_equals_float32_ring_move_for_move(name):
    from muzero_amd.replay import decode_state, state_row_bytes

    r = run(name)
    assert all(a == b for a, b in r.counts), r.counts  # num_added after every move
    per_move = np.diff([0] + [a for a, _ in r.counts])
    assert r.n > r.cap and per_move.max() > r.cap  # the ring wraps, and one move emits more items than it holds (the keep_from path)
    if r.fmt == 'frames_u8':
        assert per_move.max() >= 7  # a flush and an episode end on the same move
    (f32, prio0, org0), (cmp_, prio1, org1) = r.snap['f32'], r.snap[r.fmt]
    for f in FIELDS:
        assert f32[f].tobytes() == cmp_[f].tobytes(), f
    assert prio0.tobytes() == prio1.tobytes() and org0.tobytes() == org1.tobytes() and (org0 >= 0).all()
    rows = cmp_['state']
    assert rows.dtype == (np.uint8 if r.fmt == 'frames_u8' else np.int8) and f32['state'].dtype == np.float32
    assert rows.reshape(r.cap, -1).shape[1] == state_row_bytes(r.fmt, r.shape, r.frame_spec)
    back = decode_state(rows, r.fmt, r.frame_spec).reshape(f32['state'].shape)
    assert (bits(back) == bits(f32['state'])).all()
    assert len({s.tobytes() for s in f32['state']}) > 1
    if r.fmt == 'frames_u8':
        S, C, H, W, _ = r.frame_spec
        assert (rows[:, S * C * H * W + S:] == 0).all()  # padding bytes


def test_float32_ring_is_still_the_host_assemblers():
    """The default path: same kernels, same bytes -- the items of the float32 ring are the host EpisodeAssembler's over the same records
    (as tests/test_gpu_epilogue.py), through the wraps and the overfull moves of this run."""
    for name in ('mlp44', 'ttt'):
        r = run(name)
        ring, prio, origin = r.snap['f32']
        n, cap = r.n, r.cap
        assert n == sum(len(h) for h in r.host)
        per_env = {}
        for i in range(max(0, n - cap), n):
            per_env.setdefault(int(origin[i % cap]), []).append(i % cap)
        checked = 0
        for b, slots in per_env.items():
            items = r.host[b][len(r.host[b]) - len(slots):]
            for s, (tr, pr) in zip(slots, items):
                assert (bits(ring['state'][s]) == bits(np.asarray(tr.state, np.float32).reshape(ring['state'][s].shape))).all()
                for f in FIELDS:
                    np.testing.assert_array_equal(ring[f][s], getattr(tr, f))
                assert prio[s] == np.float32(pr)
                checked += 1
        assert checked == cap


def _learner(r, batch):
    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    net = RUNS[r.name][0]().to(dev)
    return HipLearner(net, dev, 2, batch, lr=1e-3)


def _flat_ring(rp, cap):
    ring = type(rp._ring)(rp._ring, state=rp._ring['state'].reshape(cap, -1))
    ring.state_format, ring.frame_spec = rp._ring.state_format, rp._ring.frame_spec
    return ring


@pytest.mark.parametrize('name', ['atari', 'ttt', 'gomoku5'])
def test_learner_reads_the_compact_ring_as_the_float32_ring(name):
    from forced_masks import HipTensors

    r = run(name)
    dev = torch.device('cuda', 0)
    Bn = 4 if name == 'atari' else 6
    idx = torch.tensor(([3, 0, 3, r.cap - 1, 1, 0])[:Bn], dtype=torch.int64, device=dev)  # repeats
    out = {}
    for which in ('f32', r.fmt):
        _, rp, _ = r.side[which]
        hl = _learner(r, Bn)
        ring = _flat_ring(rp, r.cap)
        loss, prio = hl.grad(ring, idx, None, Bn)
        torch.cuda.synchronize()
        res = [hl.grad_flat.cpu().numpy().copy(), loss.cpu().numpy().copy(), prio.cpu().numpy().copy(),
               HipTensors(hl).get('obs', 0, 0, (Bn, int(np.prod(r.shape))))]
        sampler = rp.device_sampler(seed=3)
        for _ in range(3):
            i, w, _ = sampler.sample(Bn)
            hl.step(ring, i, w, Bn)
        torch.cuda.synchronize()
        res.append(hl.params.cpu().numpy().copy())
        out[which] = res
        hl.close()
    a, b = out['f32'], out[r.fmt]
    assert np.isfinite(a[0]).all() and np.abs(a[0]).max() > 0
    for x, y, what in zip(a, b, ('gradient', 'loss', 'priorities', 'obs', 'weights after three steps')):
        assert x.tobytes() == y.tobytes(), what
    assert (bits(a[3]) == bits(r.snap['f32'][0]['state'][idx.cpu().numpy()].reshape(Bn, -1))).all()


def test_refusals():
    from muzero_amd import planner as pl
    from muzero_amd.hip_learner import HipLearner, LearnerError
    from muzero_amd.replay import PrioritizedReplay

    dev = torch.device('cuda', 0)

    def planner(net, B=4, **kw):
        p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=B, seed=1, num_simulations=2, **kw), 0)
        p.load_state_dict(net.state_dict())
        return p

    def replay(**kw):
        return PrioritizedReplay(16, 0.0, 0.0, np.random.RandomState(0), device='cuda', **kw)

    # device envs whose observations are not bytes
    p = planner(build_mlp(mlp_case('cartpole')), discount=0.997)
    p.attach_replay(replay(state_format='int8'), CFG, obs_shape=(4, 5))
    with pytest.raises(pl.PlannerError, match='state_format'):
        p.selfplay_reset(pl.ENV_CARTPOLE)
    p.detach_replay()
    p.close()
    at = build_conv(('atari_s', 'atari', (4, 96, 96), 6, 1, 8, 11, 11, 24))
    for kw in (dict(state_format='int8'), dict(state_format='frames_u8', frame_spec=(2, 1, 96, 96, 6))):
        p = planner(at, discount=0.997)
        p.attach_replay(replay(**kw), CFG, obs_shape=(4, 96, 96))
        with pytest.raises(pl.PlannerError, match='state_format'):
            p.selfplay_reset(pl.ENV_SYNTHETIC)
        p.detach_replay()
        p.close()
    # frames_u8 needs uint8 frames stacked on the device; and the frame_spec must be the planner's
    net = RUNS['mlp44'][0]()
    p = planner(net, discount=0.997)
    with pytest.raises(pl.PlannerError, match='frame_spec'):
        p.attach_replay(replay(state_format='frames_u8', frame_spec=(2, 1, 4, 4, 4)), CFG, obs_shape=(4, 4, 4))
    p.attach_replay(replay(state_format='frames_u8', frame_spec=(1, 3, 4, 4, 3)), CFG, obs_shape=(4, 4, 4))  # 64 elements too, other rows
    with pytest.raises(pl.PlannerError, match='frame_spec'):
        p.selfplay_reset_external(stack_history=2, is_obs_image=True, frame_shape=(1, 4, 4), frame_u8=True)
    p.detach_replay()
    p.attach_replay(replay(state_format='frames_u8', frame_spec=(2, 1, 4, 4, 3)), CFG, obs_shape=(4, 4, 4))
    with pytest.raises(pl.PlannerError, match='state_format.*frame_u8'):
        p.selfplay_reset_external(stack_history=2, is_obs_image=True, frame_shape=(1, 4, 4), frame_u8=False)
    with pytest.raises(pl.PlannerError, match='state_format.*stack_history'):
        p.selfplay_reset_external(frame_shape=(4, 4, 4))
    p.detach_replay()
    # int8 on a host-stepped env: checked state by state; env 2 shows a 0.5 in its second episode
    rp = replay(state_format='int8')
    p.attach_replay(rp, CFG, obs_shape=(4, 4, 4))
    p.selfplay_reset_external(frame_shape=(4, 4, 4))
    B, mask = 4, np.ones((4, 3), np.uint8)
    obs = (np.random.RandomState(3).uniform(size=(B, 4, 4, 4)) < 0.5).astype(np.float32)
    for m in range(2):  # every env finishes a two-move episode: 2 items each
        p.external_act(obs, mask, 1, 1, 1.0)
        p.external_commit(np.ones(B), np.full(B, m == 1))
    assert rp.num_added == 2 * B
    bad = obs.copy()
    bad[2, 1, 2, 3] = 0.5
    bad[3, 0, 0, 0] = 0.5
    p.external_act(bad, mask, 1, 1, 1.0)
    p.external_commit(np.ones(B), np.zeros(B))  # (not emitted yet)
    p.external_act(obs, mask, 1, 1, 1.0)
    with pytest.raises(pl.PlannerError, match=r'error -1: env 2: .*state_format'):
        p.external_commit(np.ones(B), np.ones(B))
    assert rp.num_added == 2 * B  # the count stays
    with pytest.raises(pl.PlannerError, match='error -3'):
        p.external_act(obs, mask, 1, 1, 1.0)
    p.selfplay_reset_external(frame_shape=(4, 4, 4))  # recovers
    for m in range(2):
        p.external_act(obs, mask, 1, 1, 1.0)
        p.external_commit(np.ones(B), np.full(B, m == 1))
    assert rp.num_added == 4 * B
    p.detach_replay()
    p.close()
    # the learner: format 2 is the conv nets', with the geometry of the net
    r = run('mlp44')
    ring = _flat_ring(r.side['frames_u8'][1], r.cap)
    idx = torch.zeros(2, dtype=torch.int64, device=dev)
    mlp = HipLearner(RUNS['mlp44'][0]().to(dev), dev, 2, 2, lr=1e-3)
    with pytest.raises(LearnerError, match='frames_u8'):
        mlp.grad(ring, idx, None, 2)
    mlp.close()
    ra = run('atari')
    hl = _learner(ra, 2)
    good = _flat_ring(ra.side['frames_u8'][1], ra.cap)
    with pytest.raises(LearnerError, match='frame_spec'):
        hl.grad(dict(good), idx, None, 2)  # a plain mapping without its frame_spec
    with pytest.raises(LearnerError, match='frame_spec'):
        hl.grad(dict(good), idx, None, 2, frame_spec=(4, 1, 96, 96, 5))
    with pytest.raises(LearnerError, match='frame_spec'):
        hl.grad(dict(good), idx, None, 2, frame_spec=(2, 1, 96, 96, 6))
    short = dict(good, state=good['state'][:, :36864].contiguous())
    with pytest.raises(LearnerError, match='state_row_bytes'):
        hl.grad(short, idx, None, 2, frame_spec=(4, 1, 96, 96, 6))
    hl.grad(dict(good), idx, None, 2, frame_spec=(4, 1, 96, 96, 6))
    torch.cuda.synchronize()
    hl.close()
