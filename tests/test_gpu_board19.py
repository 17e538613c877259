"""Board nets above 15 x 15 on an MI355X: 16 x 16 to 19 x 19 Gomoku nets (257 to 362 actions) through the conv planner -- the 19 x 19
whole-image conv build (k_conv3x3<23, 1, true, 19>), the ragged 8 x 8 tiles of the generic path, the policy head over 722 features,
the HBM trees' select over more than 256 actions and numpy's pairwise sums past 256 elements -- bit-exact against the CPU oracle and
within the fixture tolerances of the reference (tests/golden/board19_cases.npz, tools/gen_board_golden.py)."""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from board19_cases import BOARD_CASES, board_case
from fullsize_cases import BOARD_KW, FULL19  # C5's net (128 planes x 8 blocks) on a 19 x 19 board, and its search keywords
from helpers import build_conv, load_golden
from test_oracle_nets import _oracle_net

pytestmark = pytest.mark.gpu

G = load_golden('board19_cases.npz')
IDS = [c[0] for c in BOARD_CASES]


def _planner(net, num_envs, **search):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=num_envs, **search), 0)
    p.load_state_dict(net.state_dict())
    return p


def _gomoku_positions(rs, B, N, moves):
    """B Gomoku positions a few random moves into a game: observations, legal masks, players to move."""
    from muzero_amd.games import GomokuEnv

    obs, mask, cur = [], [], []
    for b in range(B):
        env = GomokuEnv(board_size=N)
        o = env.reset()
        for _ in range(moves + b % 3):
            o, _, _, _ = env.step(int(rs.choice(np.flatnonzero(env.actions_mask[:N * N]))))
        obs.append(o.astype(np.float32))
        mask.append(env.actions_mask.copy())
        cur.append(env.current_player)
    cur = np.array(cur, np.int32)
    return np.stack(obs), np.stack(mask), cur, (3 - cur).astype(np.int32)


@pytest.mark.parametrize('case', BOARD_CASES, ids=IDS)
def test_board_inference_bit_exact_vs_oracle_and_reference(oracle, case):
    net = build_conv(case)
    onet = _oracle_net(oracle, net, 'conv')
    name, A = case[0], case[3]
    obs = np.stack([G[f'{name}_{j}_obs'] for j in range(2)] + [np.random.RandomState(5).uniform(0, 1, size=case[2]).astype(np.float32)])
    B = obs.shape[0]
    p = _planner(net, B)
    hidden, pi, value = p.initial_inference(obs)
    assert pi.shape == (B, A)
    for b in range(B):
        oh, _, opi, ov = onet.initial_inference(obs[b])
        np.testing.assert_array_equal(hidden[b], oh)
        np.testing.assert_array_equal(pi[b], opi)
        assert value[b] == np.float32(ov)
    for j in range(2):  # the reference's chain: its own hidden state into each step
        pre = f'{name}_{j}'
        np.testing.assert_allclose(hidden[j], G[f'{pre}_init_hidden'].reshape(-1), rtol=2e-5, atol=2e-6)
        np.testing.assert_allclose(pi[j], G[f'{pre}_init_pi'], rtol=2e-5, atol=1e-7)
        np.testing.assert_allclose(value[j], G[f'{pre}_init_value'], rtol=2e-4, atol=2e-4)
        for t, a in enumerate(G[f'{pre}_actions']):
            h_ref = G[f'{pre}_init_hidden'] if t == 0 else G[f'{pre}_rec_hidden'][t - 1]
            h2, r, pi2, v2 = p.recurrent_inference(h_ref.reshape(1, -1).astype(np.float32), np.array([a], np.int32))
            oh2, orw, opi2, ov2 = onet.recurrent_inference(h_ref, int(a))
            np.testing.assert_array_equal(h2[0], oh2)
            np.testing.assert_array_equal(pi2[0], opi2)
            assert r[0] == np.float32(orw) and v2[0] == np.float32(ov2)
            np.testing.assert_allclose(h2[0], G[f'{pre}_rec_hidden'][t].reshape(-1), rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(pi2[0], G[f'{pre}_rec_pi'][t], rtol=2e-5, atol=1e-7)
            np.testing.assert_allclose(v2[0], G[f'{pre}_rec_value'][t], rtol=2e-4, atol=2e-4)
            np.testing.assert_allclose(r[0], G[f'{pre}_rec_reward'][t], rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize('case', BOARD_CASES, ids=IDS)
def test_board_search_matches_reference_fixture_and_oracle(oracle, case):
    """The reference's uct_search (40 simulations, alpha 0.03 over 362 / 257 actions) with its recorded draws: visits and action equal
    the fixture; every output equals the oracle's."""
    from test_oracle_board19 import search_config

    net = build_conv(case)
    onet = _oracle_net(oracle, net, 'conv')
    name, A = case[0], case[3]
    pre = f'{name}_search'
    S = int(G[f'{pre}_sims'])
    p = _planner(net, 1, num_simulations=S, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0),
                 root_dirichlet_alpha=float(G[f'{pre}_alpha']), root_exploration_eps=float(G[f'{pre}_eps']))
    args = (int(G[f'{pre}_cur_player']), int(G[f'{pre}_opp_player']), float(G[f'{pre}_temperature']), bool(G[f'{pre}_deterministic']))
    u_tie = G[f'{pre}_u_tie'][:4 * S + 8]
    r = p.search(G[f'{pre}_obs'][None], G[f'{pre}_mask'][None], *args, noise=G[f'{pre}_noise'][None], u_tie=u_tie[None],
                 u_final=np.array([float(G[f'{pre}_u_final'])]))
    np.testing.assert_array_equal(r['visits'][0], G[f'{pre}_visits'])
    assert r['action'][0] == int(G[f'{pre}_out_action'])
    np.testing.assert_array_equal(r['pi'][0], G[f'{pre}_out_pi'])
    o = oracle.uct_search(search_config(oracle, name, A), onet, G[f'{pre}_obs'], G[f'{pre}_mask'], *args, noise=G[f'{pre}_noise'], u_tie=u_tie,
                          u_final=float(G[f'{pre}_u_final']))
    np.testing.assert_array_equal(r['visits'][0], o['visits'])
    np.testing.assert_array_equal(r['pi'][0], o['pi'])
    assert r['action'][0] == o['action'] and r['root_value'][0] == o['root_value']


@pytest.mark.parametrize('N,P,B,S', [(16, 16, 7, 12), (17, 8, 6, 10), (18, 16, 5, 10), (19, 16, 9, 12)])
def test_board_batched_search_bit_exact_vs_oracle(oracle, N, P, B, S):
    """Lock-step envs on every board size past 15 x 15 (ragged 8 x 8 tiles at 17 and 18, four whole tiles at 16, the generic path at
    19 x 19 with 16 planes): every env equals an independent oracle search, stochastic and deterministic."""
    case = (f'board{N}', 'board', (9, N, N), N * N + 1, 1, P, 1, 1, 50 + N)
    net = build_conv(case)
    onet = _oracle_net(oracle, net, 'conv')
    A = case[3]
    p = _planner(net, B, num_simulations=S, **BOARD_KW)
    rs = np.random.RandomState(N)
    obs, mask, cur, opp = _gomoku_positions(rs, B, N, 3)
    temp = rs.choice([1.0, 0.5, 0.1], size=B)
    noise = rs.dirichlet(np.full(A, 0.03), size=B)
    u_tie = rs.rand(B, 4 * S + 8)
    u_final = rs.rand(B)
    ocfg = oracle.make_config(A, S, 1.0, True, (-1.0, 1.0), 0.03, 0.25)
    for det in (False, True):
        r = p.search(obs, mask, cur, opp, temp, det, noise=None if det else noise, u_tie=u_tie, u_final=u_final)
        o = oracle.uct_search_batch(ocfg, onet, obs, mask.astype(np.uint8), cur, opp, temp, det, noise=None if det else noise, u_tie=u_tie,
                                    u_final=u_final)
        np.testing.assert_array_equal(r['visits'], o['visits'])
        np.testing.assert_array_equal(r['pi'], o['pi'])
        np.testing.assert_array_equal(r['action'], o['action'])
        np.testing.assert_array_equal(r['root_value'], o['root_value'])


def _full_size_run(B=2, S=16):
    """The full-size 19 x 19 net: inference and one search with fixed draws (used in this process and in the MZ_CONV_SPEC children)."""
    net = build_conv(FULL19)
    A = FULL19[3]
    rs = np.random.RandomState(19)
    obs, mask, cur, opp = _gomoku_positions(rs, B, 19, 6)
    actions = rs.randint(0, A, size=B).astype(np.int32)
    noise = rs.dirichlet(np.full(A, 0.03), size=B)
    u_tie = rs.rand(B, 4 * S + 8)
    u_final = rs.rand(B)
    p = _planner(net, B, num_simulations=S, **BOARD_KW)
    hidden, pi, value = p.initial_inference(obs)
    h2, reward, pi2, value2 = p.recurrent_inference(hidden, actions)
    r = p.search(obs, mask, cur, opp, 1.0, False, noise=noise, u_tie=u_tie, u_final=u_final)
    out = dict(obs=obs, mask=mask, cur=cur, opp=opp, actions=actions, noise=noise, u_tie=u_tie, u_final=u_final, hidden=hidden, pi=pi, value=value,
               h2=h2, reward=reward, pi2=pi2, value2=value2, visits=r['visits'], spi=r['pi'], action=r['action'], root=r['root_value'])
    p.close()
    return net, out


def test_full_size_19x19_spot_check_vs_oracle(oracle):
    """128 planes x 8 blocks at 19 x 19 (every tower conv on the whole-image build), 2 envs x 16 simulations: inference and search
    bit-exact against the oracle (~1 s of scalar CPU per oracle simulation at this size)."""
    net, r = _full_size_run()
    onet = _oracle_net(oracle, net, 'conv')
    for b in range(2):
        oh, _, opi, ov = onet.initial_inference(r['obs'][b])
        np.testing.assert_array_equal(r['hidden'][b], oh)
        np.testing.assert_array_equal(r['pi'][b], opi)
        assert r['value'][b] == np.float32(ov)
        oh2, orw, opi2, ov2 = onet.recurrent_inference(oh, int(r['actions'][b]))
        np.testing.assert_array_equal(r['h2'][b], oh2)
        np.testing.assert_array_equal(r['pi2'][b], opi2)
        assert r['reward'][b] == np.float32(orw) and r['value2'][b] == np.float32(ov2)
    ocfg = oracle.make_config(362, 16, 1.0, True, (-1.0, 1.0), 0.03, 0.25)
    o = oracle.uct_search_batch(ocfg, onet, r['obs'], r['mask'].astype(np.uint8), r['cur'], r['opp'], 1.0, False, noise=r['noise'], u_tie=r['u_tie'],
                                u_final=r['u_final'])
    np.testing.assert_array_equal(r['visits'], o['visits'])
    np.testing.assert_array_equal(r['spi'], o['pi'])
    np.testing.assert_array_equal(r['action'], o['action'])
    np.testing.assert_array_equal(r['root'], o['root_value'])


def test_full_size_19x19_tuned_and_generic_builds_agree(tmp_path):
    """MZ_CONV_SPEC=1 (the 19 x 19 whole-image build) and MZ_CONV_SPEC=0 (nine ragged 8 x 8 tiles per image) give identical inference
    and search outputs.  The switch is read once per process: one fresh child process per build."""
    outs = []
    for spec in ('1', '0'):
        path = str(tmp_path / f'spec{spec}.npz')
        code = ('import sys, numpy as np; sys.path.insert(0, %r); import test_gpu_board19 as t; _, r = t._full_size_run(); np.savez(%r, **r)'
                % (os.path.dirname(os.path.abspath(__file__)), path))
        env = dict(os.environ, MZ_CONV_SPEC=spec)
        res = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
        outs.append(np.load(path))
    for k in ('hidden', 'pi', 'value', 'h2', 'reward', 'pi2', 'value2', 'visits', 'spi', 'action', 'root'):
        np.testing.assert_array_equal(outs[0][k], outs[1][k], err_msg=k)


def test_gomoku_19x19_selfplay_search_equals_oracle(oracle):
    """Device Gomoku 19 x 19 self-play (k_env_step on 361 points, 362-action policies in the record ring): every move's recorded search
    input and captured Philox draws through the oracle env + oracle search give the same policy, root value and action."""
    from test_gpu_selfplay import selfplay_search_vs_oracle

    selfplay_search_vs_oracle(oracle, 'gomoku', board_case('board19'), 8, 8, 6, expect_resets=False)


def test_gomoku_19x19_epilogue_items_match_host_assembler():
    """The device epilogue at 19 x 19: items with a 9 x 361 state, int16 actions and 362 pi_prob values equal the host EpisodeAssembler
    fed with the same records; 368 moves end at least one game per env (a full board ends one)."""
    from test_gpu_epilogue import _compare
    from muzero_amd import planner as pl
    from muzero_amd.pipeline import EpisodeAssembler
    from muzero_amd.replay import PrioritizedReplay

    cfg = types.SimpleNamespace(is_board_game=True, acc_seq_length=9999, unroll_steps=5, td_steps=0, discount=1.0)
    net = build_conv(board_case('board19'))
    B, moves, chunk = 4, 368, 16
    p = _planner(net, B, seed=9, num_simulations=2, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0), root_dirichlet_alpha=0.03)
    rp = PrioritizedReplay(4096, 0.0, 0.0, np.random.RandomState(0), device='cuda')
    origin = p.attach_replay(rp, cfg, obs_shape=(9, 19, 19), with_origin=True)
    assert rp._ring['action'].dtype == torch.int16
    p.selfplay_reset(pl.ENV_GOMOKU)
    asm = [EpisodeAssembler(cfg, 1, (9, 19, 19)) for _ in range(B)]
    host = [[] for _ in range(B)]
    for lo in range(0, moves, chunk):
        p.selfplay_step(-1.0, chunk)
        rec = p.selfplay_read(chunk)
        for b in range(B):
            host[b].extend(asm[b].feed({k: v[:, b:b + 1] for k, v in rec.items()}))
    n = rp.num_added
    assert n == sum(len(h) for h in host) and n > 0 and all(len(h) > 0 for h in host)
    assert _compare(rp, origin.cpu().numpy(), host, n) == n
    ring = {k: v.cpu().numpy() for k, v in rp._ring.items()}
    assert ring['pi_prob'].shape[1:] == (5, 362) and ring['state'][0].size == 9 * 361
    assert ring['action'][:n].max() > 255  # stone positions past 255 were played and stored intact
    p.close()


def test_gomoku_19x19_host_envs_equal_device_env_records():
    """MZ_ENV_EXTERNAL with games.GomokuEnv(board_size=19): every record equals the device env's."""
    from muzero_amd import games
    from muzero_amd import planner as pl

    B, M, S = 4, 20, 4
    net = build_conv(board_case('board19'))
    kw = dict(num_simulations=S, seed=5, discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0))
    pd = _planner(net, B, **kw)
    pd.selfplay_reset(pl.ENV_GOMOKU)
    pd.selfplay_step(-1.0, M)
    dev = pd.selfplay_read(M)
    pd.close()
    ph = _planner(net, B, **kw)
    ph.selfplay_reset_external(frame_shape=(9, 19, 19), temp_switch_steps=30)
    envs = [games.GomokuEnv(board_size=19) for _ in range(B)]
    obs = [e.reset() for e in envs]
    for m in range(M):
        a = ph.external_act(np.stack(obs), np.stack([e.actions_mask for e in envs]), [e.current_player for e in envs],
                            [e.opponent_player for e in envs], -1.0)
        rew, done = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        for i, e in enumerate(envs):
            obs[i], rew[i], d, _ = e.step(int(a[i]))
            if d:
                obs[i] = e.reset()
            done[i] = d
        ph.external_commit(rew, done)
    host = ph.selfplay_read(M)
    ph.close()
    assert dev['pi'].shape[-1] == 362
    for k in dev:
        assert np.array_equal(dev[k], host[k]), k


def test_python_surface_takes_19x19_board_nets():
    """mcts.uct_search / batched_uct_search and the module's initial / recurrent inference (network.InferenceEngine) on a 19 x 19 net,
    with no special casing by the caller."""
    from muzero_amd import mcts
    from muzero_amd.config import make_gomoku_config
    from muzero_amd.games import GomokuEnv

    net = build_conv(board_case('board19'))
    dev = torch.device('cuda', 0)
    cfg = make_gomoku_config(use_tensorboard=False)
    cfg.num_simulations = 8
    env = GomokuEnv(board_size=19)
    obs = env.reset()
    action, pi, root = mcts.uct_search(obs, net, dev, cfg, 0.0, env.actions_mask, env.current_player, env.opponent_player, deterministic=True)
    assert pi.shape == (362,) and env.actions_mask[action] and abs(pi.sum() - 1.0) < 1e-12
    acts, pis, roots = mcts.batched_uct_search(np.stack([obs, obs]), net, dev, cfg, 1.0, np.stack([env.actions_mask] * 2), 1, 2)
    assert pis.shape == (2, 362) and acts.shape == (2,)
    out = net.initial_inference(torch.from_numpy(obs.astype(np.float32))[None].to(dev))
    assert out.hidden_state.shape == (8, 19, 19) and out.pi_probs.shape == (362,)
    out2 = net.recurrent_inference(torch.from_numpy(out.hidden_state)[None].to(dev), torch.tensor([[360]]))
    assert out2.pi_probs.shape == (362,) and np.isfinite(out2.value)


def test_20x20_board_net_is_refused():
    from muzero_amd import network
    from muzero_amd import planner as pl

    net = network.MuZeroBoardGameNet((9, 20, 20), 401, 1, 8)
    with pytest.raises(pl.PlannerError, match='361'):
        pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=2), 0)
