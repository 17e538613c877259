"""The opt-in split-bf16 conv path (mz_config.conv_precision = MZ_CONV_BF16X3, muzero_amd/csrc/mz_conv_split.h) on the GPU.

The path is NOT bit-equal to the oracle: it is held to the reference -- at the bars tests/test_oracle_nets.py holds the oracle to
the reference (toy nets), to the oracle's float32 outputs at the same bars where no fixture exists, and to the full-size fixtures
through tests/test_oracle_fullsize.py's checks -- and to itself bit for bit across batches, rows, runs and kernel builds."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fullsize_cases import FULL, full_case
from helpers import build_conv, build_mlp, conv_case, load_golden, mlp_case
from test_oracle_fullsize import check_inference, check_search, hidden_in, load, search_kwargs
from test_oracle_nets import HID_TOL, PI_TOL, VAL_TOL, _oracle_net

pytestmark = pytest.mark.gpu

NETS = load_golden('net_cases.npz')
BOARD_KW = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.25, root_exploration_eps=0.25)
# shapes without a fixture: name, kind, input_shape, A, blocks, planes, value_support, reward_support, seed
EXTRA = {
    'p48': ('p48', 'board', (5, 7, 7), 50, 2, 48, 1, 1, 61),       # planes not a multiple of 32, odd side
    'w15': ('w15', 'board', (9, 15, 15), 226, 2, 64, 1, 1, 62),    # the whole-image 15 x 15 build
    'w19': ('w19', 'board', (9, 19, 19), 362, 2, 64, 1, 1, 63),    # the whole-image 19 x 19 build
    'g9': ('g9', 'board', (9, 9, 9), 82, 2, 32, 1, 1, 64),         # device Gomoku 9 x 9
}


def _planner(net, num_envs, precision='bf16x3', seed=1, **search):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=num_envs, seed=seed, conv_precision=precision, **search), 0)
    p.load_state_dict(net.state_dict())
    return p


# ------------------------------------------------------------------------------------------ 1. toy sizes against the reference
@pytest.mark.parametrize('B', [1, 5, 64])
@pytest.mark.parametrize('g', ['board3', 'board5', 'board9'])
def test_toy_inference_matches_reference_fixture(g, B):
    """9 pixels in an 8 x 8 tile, 81 pixels in four ragged tiles, 8 / 16 planes and 9 input channels against K = 32, dense action planes
    (8 planes) and sparse action terms (16 planes): the fixture rows inside batches of 1, 5 and 64."""
    case = conv_case(g)
    net = build_conv(case)
    p = _planner(net, B)
    rs = np.random.RandomState(B)
    for j in range(2):
        pre = f'conv_{g}_{j}'
        row = (3 * j + 1) % B
        obs = rs.uniform(0, 1, size=(B,) + tuple(case[2])).astype(np.float32)
        obs[row] = NETS[f'{pre}_obs']
        hidden, pi, value = p.initial_inference(obs)
        np.testing.assert_allclose(hidden[row], NETS[f'{pre}_init_hidden'].reshape(-1), **HID_TOL)
        np.testing.assert_allclose(pi[row], NETS[f'{pre}_init_pi'], **PI_TOL)
        np.testing.assert_allclose(value[row], NETS[f'{pre}_init_value'], **VAL_TOL)
        acts = NETS[f'{pre}_actions']
        n = len(acts)
        hin = np.concatenate([NETS[f'{pre}_init_hidden'].reshape(1, -1), NETS[f'{pre}_rec_hidden'].reshape(n, -1)[:-1]])
        for t in range(n):  # step t of the fixture at `row`, the other rows: hidden states of this net with random actions
            hb = hidden[rs.permutation(B)]
            ab = rs.randint(0, case[3], size=B).astype(np.int32)
            hb[row], ab[row] = hin[t], acts[t]
            h, r, pi2, v = p.recurrent_inference(hb, ab)
            np.testing.assert_allclose(h[row], NETS[f'{pre}_rec_hidden'].reshape(n, -1)[t], **HID_TOL)
            np.testing.assert_allclose(r[row], np.asarray(NETS[f'{pre}_rec_reward']).reshape(-1)[t], **VAL_TOL)
            np.testing.assert_allclose(v[row], np.asarray(NETS[f'{pre}_rec_value']).reshape(-1)[t], **VAL_TOL)
            np.testing.assert_allclose(pi2[row], NETS[f'{pre}_rec_pi'][t], **PI_TOL)
    p.close()


# ------------------------------------------------------------------------------------------ 2. other shapes against the oracle
def _io(case, B, seed=5):
    rs = np.random.RandomState(seed)
    obs = (rs.rand(B, *case[2]) < 0.3).astype(np.float32)
    actions = rs.randint(0, case[3], size=B).astype(np.int32)
    return obs, actions


@pytest.mark.parametrize('g,build', [('p48', 'shape-generic'), ('w15', 'SIDE=15'), ('w19', 'SIDE=19')])
def test_inference_matches_oracle_fp32_within_reference_bars(oracle, g, build):
    """The oracle's float32 outputs at the bars the oracle itself is held to the reference at.  The hidden state is normalised to [0, 1] and
    the value / reward of these seeded nets are O(0.1 .. 1) (checked on the CPU when the seeds were fixed; asserted below), so the
    absolute parts of the bars bind."""
    case = EXTRA[g]
    net = build_conv(case)
    onet = _oracle_net(oracle, net, 'conv')
    B = 3
    p = _planner(net, B)
    obs, actions = _io(case, B)
    hidden, pi, value = p.initial_inference(obs)
    h2, reward, pi2, value2 = p.recurrent_inference(hidden, actions)
    assert build in p.describe() and 'conv_precision=bf16x3' in p.describe()
    for b in range(B):
        oh, _, opi, ov = onet.initial_inference(obs[b])
        assert oh.max() == 1.0 and 0.01 < abs(float(ov)) < 10.0
        np.testing.assert_allclose(hidden[b], oh, **HID_TOL)
        np.testing.assert_allclose(pi[b], opi, **PI_TOL)
        np.testing.assert_allclose(value[b], ov, **VAL_TOL)
        oh2, orw, opi2, ov2 = onet.recurrent_inference(hidden[b], int(actions[b]))
        np.testing.assert_allclose(h2[b], oh2, **HID_TOL)
        np.testing.assert_allclose(reward[b], orw, **VAL_TOL)
        np.testing.assert_allclose(value2[b], ov2, **VAL_TOL)
        np.testing.assert_allclose(pi2[b], opi2, **PI_TOL)
    p.close()


# ------------------------------------------------------------------------------------------ 3. full size against the reference
def _fullsize_inference(p, G, name, case, B, rows):
    """tests/test_gpu_fullsize.py's driver: the two fixture observations at `rows` of a batch of B, seeded random rows elsewhere."""
    shape, A = case[2], case[3]
    rs = np.random.RandomState(B)
    obs = (rs.rand(B, *shape) < 0.3).astype(np.float32)
    for j, b in enumerate(rows):
        obs[b] = G[f'{name}_{j}_obs'].astype(np.float32)
    hidden, pi, value = p.initial_inference(obs)
    got = {(j, -1): (hidden[b].copy(), 0.0, pi[b].copy(), value[b]) for j, b in enumerate(rows)}
    steps = max(len(G[f'{name}_{j}_actions']) for j in range(2))
    for t in range(steps):
        hin = hidden[rs.permutation(B)]
        act = rs.randint(0, A, size=B).astype(np.int32)
        live = [(j, b) for j, b in enumerate(rows) if t < len(G[f'{name}_{j}_actions'])]
        for j, b in live:
            hin[b] = hidden_in(G, name, j, t)
            act[b] = int(G[f'{name}_{j}_actions'][t])
        h2, r, pi2, v2 = p.recurrent_inference(hin, act)
        for j, b in live:
            got[(j, t)] = (h2[b].copy(), r[b], pi2[b].copy(), v2[b])
    return got


@pytest.mark.parametrize('name', ['c5', 'c5_19'])
def test_fullsize_inference_matches_reference(name):
    """128 planes x 8 blocks in a batch of 256: every recorded initial and recurrent output within max(toy bar, 4 * e32) of the reference."""
    case = full_case(name)
    G = load(name)
    B = FULL[name][1]
    p = _planner(build_conv(case), B)
    got = _fullsize_inference(p, G, name, case, B, (1, B - 2))
    assert len(got) >= 4
    for (j, t), out in got.items():
        check_inference(G, name, j, t, out)
    assert 'whole image' in p.describe()
    p.close()


@pytest.mark.parametrize('name', ['c5', 'c5_19'])
def test_fullsize_search_matches_reference(name):
    """The reference's recorded search (kept only where its float32 and float64 searches agree) at a middle row of 16 envs: visits,
    policy and action equal, root value within 1e-4."""
    case = full_case(name)
    A = case[3]
    G = load(name)
    g = f'{name}_search'
    kw = search_kwargs(G, name)
    S, B = kw['num_simulations'], 16
    row = B // 2 - 1
    p = _planner(build_conv(case), B, **kw)
    rs = np.random.RandomState(S)
    rep = lambda x: np.repeat(np.asarray(x)[None], B, axis=0)  # noqa: E731
    noise = rs.dirichlet(np.full(A, kw['root_dirichlet_alpha']), size=B)
    u_tie = rs.rand(B, 4 * S + 8)
    u_final = rs.rand(B)
    noise[row], u_tie[row], u_final[row] = G[f'{g}_noise'], G[f'{g}_u_tie'][:4 * S + 8], float(G[f'{g}_u_final'])
    r = p.search(rep(G[f'{g}_obs'].astype(np.float32)), rep(G[f'{g}_mask']), int(G[f'{g}_cur_player']), int(G[f'{g}_opp_player']),
                 float(G[f'{g}_temperature']), bool(G[f'{g}_deterministic']), noise=noise, u_tie=u_tie, u_final=u_final)
    check_search(G, name, r['visits'][row], r['pi'][row], int(r['action'][row]), float(r['root_value'][row]))
    p.close()


# ------------------------------------------------------------------------------------------ 4. rows, batches, runs, builds
def _row_outputs(g):
    """The outputs of three fixed observations of net `g`, placed at other rows of batches of 3 and 256; asserts that batch, row and run do
    not change a bit, returns the outputs."""
    case = EXTRA[g]
    net = build_conv(case)
    obs3, act3 = _io(case, 3, seed=9)
    p = _planner(net, 256)
    ref = None
    for B, rows in ((3, (0, 1, 2)), (3, (2, 0, 1)), (256, (5, 130, 255)), (256, (255, 0, 77))):
        obs, act = _io(case, B, seed=B)
        obs[list(rows)], act[list(rows)] = obs3, act3
        for run in range(2):
            hidden, pi, value = p.initial_inference(obs)
            h2, reward, pi2, value2 = p.recurrent_inference(hidden, act)
            out = [x[list(rows)] for x in (hidden, pi, value, h2, reward, pi2, value2)]
            if ref is None:
                ref = out
            for x, y in zip(out, ref):
                np.testing.assert_array_equal(x, y, err_msg=f'{g}: batch {B}, rows {rows}, run {run}')
    desc = p.describe()
    p.close()
    return ref, desc


@pytest.mark.parametrize('g', ['w15', 'w19'])
def test_rows_batches_runs_and_builds_agree_bit_for_bit(g, tmp_path):
    ref, desc = _row_outputs(g)
    assert 'whole image' in desc
    out = str(tmp_path / 'generic.npz')
    env = dict(os.environ, MZ_CONV_SPEC='0')  # read once per process: the shape-generic build in a child
    r = subprocess.run([sys.executable, os.path.abspath(__file__), g, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    G = np.load(out)
    assert 'shape-generic' in str(G['describe'])
    for i, x in enumerate(ref):
        np.testing.assert_array_equal(G[f'o{i}'], x, err_msg=f'{g}: output {i}, generic vs whole-image build')


# ------------------------------------------------------------------------------------------ 5. everything above the conv
def _selfplay_records(seed, B, M, S):
    from muzero_amd import planner as pl

    p = _planner(build_conv(EXTRA['g9']), B, seed=seed, num_simulations=S, **dict(BOARD_KW, root_dirichlet_alpha=0.03))
    p.selfplay_reset(pl.ENV_GOMOKU)
    p.selfplay_step(-1.0, M)
    rec, cnt = p.selfplay_read(M), p.selfplay_counters()
    p.close()
    return rec, cnt


def test_device_gomoku_selfplay(oracle):
    """Gomoku 9 x 9, 32 planes x 2 blocks, 16 envs x 8 moves x 16 simulations with Philox draws: the records replay through the oracle's
    BoardEnv (legal moves, observations, players), policies are distributions over the legal moves, the counters add up, and a second
    run from the same seed records the same."""
    B, M, S = 16, 8, 16
    rec, cnt = _selfplay_records(7, B, M, S)
    assert cnt['env_steps'] == B * M and cnt['simulations'] == B * M * S
    assert cnt['episodes'] == int(rec['done'].sum())
    for b in range(B):
        env = oracle.BoardEnv(9, 4, 5)
        obs = env.reset()
        for m in range(M):
            np.testing.assert_array_equal(rec['obs'][m, b].reshape(9, 9, 9), obs.astype(np.float32))
            assert rec['player'][m, b] == env.current_player
            a = int(rec['action'][m, b])
            assert env.actions_mask[a], 'sampled action must be legal'
            pi = rec['pi'][m, b]
            assert abs(pi.sum() - 1.0) < 1e-12 and (pi[~env.actions_mask] == 0).all()
            assert np.isfinite(rec['root_value'][m, b])
            obs, r, done = env.step(a)
            assert r == rec['reward'][m, b] and done == bool(rec['done'][m, b])
            if done:  # (action 81 resigns: an episode may end early; the device env resets itself)
                env = oracle.BoardEnv(9, 4, 5)
                obs = env.reset()
    rec2, cnt2 = _selfplay_records(7, B, M, S)
    assert cnt2 == cnt
    for k in rec:
        np.testing.assert_array_equal(rec[k], rec2[k], err_msg=k)


def test_arena_of_two_split_planners():
    """8 games of 9 x 9 Gomoku between two split planners, to the end: a consistent tally."""
    from helpers import seeded_state_dict
    from muzero_amd import planner as pl

    B = 8
    net_p, net_q = build_conv(EXTRA['g9']), build_conv(EXTRA['g9'])
    net_q.load_state_dict(seeded_state_dict(net_q, 164))
    p = _planner(net_p, B, seed=3, num_simulations=6, **BOARD_KW)
    q = _planner(net_q, B, seed=4, num_simulations=6, **BOARD_KW)
    p.arena_reset(pl.ENV_GOMOKU, q, opening_plies=2)
    p.arena_step(81)
    res = p.arena_result()
    assert res['live'] == 0
    assert res['challenger_wins'] + res['opponent_wins'] + res['draws'] == B
    assert (res['winner'] != pl.ARENA_UNFINISHED).all() and (res['length'] >= 1).all() and (res['length'] <= 81).all()  # (action 81 resigns: a game may end at any ply)
    assert res['finished_plies'] == int(res['length'].sum())
    assert res['challenger_wins'] == int((res['winner'] == pl.ARENA_WIN_CHALLENGER).sum())
    np.testing.assert_array_equal(res['ret'], np.where(res['winner'] == pl.ARENA_WIN_CHALLENGER, 1.0, np.where(res['winner'] == pl.ARENA_WIN_OPPONENT, -1.0, 0.0)))
    p.close()
    q.close()


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    import ctypes as C

    from muzero_amd import planner as pl

    lib = pl.load_library()
    for net, word in ((build_mlp(mlp_case('tictactoe')), 'MZ_NET_MLP'), (build_conv(conv_case('atari_s')), 'MZ_NET_ATARI')):
        cfg = pl.make_mz_config(net.planner_spec(), None, num_envs=4, conv_precision='bf16x3')
        h = C.c_void_p()
        assert lib.mz_planner_create(C.byref(cfg), 0, C.byref(h)) == -1
        msg = lib.mz_last_error().decode()
        assert 'conv_precision' in msg and word in msg
    cfg = pl.make_mz_config(build_conv(conv_case('board3')).planner_spec(), None, num_envs=4)
    cfg.conv_precision = 2
    h = C.c_void_p()
    assert lib.mz_planner_create(C.byref(cfg), 0, C.byref(h)) == -1
    assert 'conv_precision' in lib.mz_last_error().decode()
    # an arena whose planners differ in precision
    net = build_conv(EXTRA['g9'])
    p = _planner(net, 8, seed=1, num_simulations=4, **BOARD_KW)
    q = _planner(net, 8, precision='f32', seed=2, num_simulations=4, **BOARD_KW)
    assert lib.mz_arena_reset(p.h, pl.ENV_GOMOKU, pl.ARENA_PLANNER, q.h, 0, None) == -1
    assert lib.mz_arena_reset(q.h, pl.ENV_GOMOKU, pl.ARENA_PLANNER, p.h, 0, None) == -1
    p.close()
    q.close()


# ------------------------------------------------------------------------------------------ 7. the default is untouched
def test_default_precision_stays_bit_equal_to_the_oracle(oracle):
    """A float32 planner created next to a split one: board5 bit for bit against the oracle, the project's standing contract."""
    case = conv_case('board5')
    net = build_conv(case)
    onet = _oracle_net(oracle, net, 'conv')
    B = 7
    ps = _planner(net, B)
    pf = _planner(net, B, precision='f32')
    obs = np.random.RandomState(7).uniform(0, 1, size=(B,) + tuple(case[2])).astype(np.float32)
    actions = np.random.RandomState(8).randint(0, case[3], size=B).astype(np.int32)
    ps.initial_inference(obs)
    hidden, pi, value = pf.initial_inference(obs)
    ps.recurrent_inference(hidden, actions)
    h2, reward, pi2, value2 = pf.recurrent_inference(hidden, actions)
    assert 'conv_precision=f32' in pf.describe()
    for b in range(B):
        oh, _, opi, ov = onet.initial_inference(obs[b])
        np.testing.assert_array_equal(hidden[b], oh)
        np.testing.assert_array_equal(pi[b], opi)
        assert value[b] == np.float32(ov)
        oh2, orw, opi2, ov2 = onet.recurrent_inference(oh, int(actions[b]))
        np.testing.assert_array_equal(h2[b], oh2)
        np.testing.assert_array_equal(pi2[b], opi2)
        assert reward[b] == np.float32(orw) and value2[b] == np.float32(ov2)
    ps.close()
    pf.close()


if __name__ == '__main__':  # child of test_rows_batches_runs_and_builds_agree_bit_for_bit: <net> <out.npz>
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    outs, description = _row_outputs(sys.argv[1])
    np.savez(sys.argv[2], describe=description, **{f'o{i}': x for i, x in enumerate(outs)})
