"""The HIP path at the full sizes -- C4 (Atari 8 x 96 x 96, 512 envs), C5 (Gomoku 15 x 15, 256 envs), C5-19 (19 x 19, 256 envs), each 128
planes x 8 residual blocks -- against the reference outputs of tests/golden/fullsize_<net>.npz (tools/gen_fullsize_golden.py), inside
batches that reach the tuned builds: k_conv3x3<15, 1, true, 15[, true]> (whole 15 x 15 images), k_conv3x3<23, 1, true, 19> (whole
19 x 19 images), k_conv3x3<12, 2, false, 48> and k_conv3x3<9, 2, false, 24> (the Atari representation's 48 x 48 and 24 x 24 layers, which
need >= 1024 workgroups in the launch: 43 and 128 envs) and k_res_tower (the 6 x 6 Atari towers).  profiles/fullsize/kernel_stats.csv is
the kernel list of one traced run of this file.

Tolerances: those of tests/test_oracle_fullsize.py -- rtol of the toy-size tests, atol = max(theirs, 4 * e32[kind]) with e32 the
reference's own float32-vs-float64 distance stored in the fixture; searches: visits, policy and action equal, root value within
1e-4 * max(1, |v|).  The oracle is not needed here: tests/test_oracle_fullsize.py holds it to the same fixtures, and the spot checks of
tests/test_gpu_conv.py / tests/test_gpu_board19.py hold the HIP path to the oracle bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fullsize_cases import FULL, FULL_CASES
from helpers import build_conv
from test_oracle_fullsize import check_inference, check_search, hidden_in, load, search_kwargs

pytestmark = pytest.mark.gpu

IDS = [c[0] for c in FULL_CASES]
SEARCH_ENVS = {'c4': 128, 'c5': 16, 'c5_19': 16}  # C4: enough workgroups for two channel tiles per wave on the 48 x 48 and 24 x 24 layers


def _planner(net, num_envs, **search):
    from muzero_amd import planner as pl

    p = pl.Planner(pl.make_mz_config(net.planner_spec(), None, num_envs=num_envs, **search), 0)
    p.load_state_dict(net.state_dict())
    return p


def _random_obs(rs, kind, n, shape):
    if kind == 'atari':
        return rs.randint(0, 256, size=(n,) + tuple(shape)).astype(np.float32)
    return (rs.rand(n, *shape) < 0.3).astype(np.float32)


def _inference(p, G, name, case, B, rows):
    """Initial inference and the recorded recurrent steps with the two fixture observations at `rows` of a batch of B, the other rows seeded
    random; returns the fixture rows' outputs as {(j, step): (hidden, reward, pi, value)}."""
    kind, shape, A = case[1], case[2], case[3]
    rs = np.random.RandomState(B)
    obs = _random_obs(rs, kind, B, shape)
    for j, b in enumerate(rows):
        obs[b] = G[f'{name}_{j}_obs'].astype(np.float32)
    hidden, pi, value = p.initial_inference(obs)
    assert pi.shape == (B, A)
    got = {(j, -1): (hidden[b].copy(), 0.0, pi[b].copy(), value[b]) for j, b in enumerate(rows)}
    steps = max(len(G[f'{name}_{j}_actions']) for j in range(2))
    for t in range(steps):
        hin = hidden[rs.permutation(B)]  # the other rows: hidden states of this net
        act = rs.randint(0, A, size=B).astype(np.int32)
        live = [(j, b) for j, b in enumerate(rows) if t < len(G[f'{name}_{j}_actions'])]
        for j, b in live:
            hin[b] = hidden_in(G, name, j, t)
            act[b] = int(G[f'{name}_{j}_actions'][t])
        h2, r, pi2, v2 = p.recurrent_inference(hin, act)
        for j, b in live:
            got[(j, t)] = (h2[b].copy(), r[b], pi2[b].copy(), v2[b])
    return got


@pytest.mark.parametrize('case', FULL_CASES, ids=IDS)
def test_fullsize_inference_in_batch_matches_reference(case):
    """The fixture observations at rows 1 and B - 2 of a batch of the BASELINE env count: every initial and recurrent output against the
    reference; then the same observations in a ragged batch of 3 (another launch geometry: one channel tile per wave on the Atari
    layers, other workgroup groupings): bit-equal to the full-batch rows -- the output of an env does not depend on its neighbours or on
    the launch geometry."""
    name = case[0]
    G = load(name)
    B = FULL[name][1]
    net = build_conv(case)
    p = _planner(net, B)
    full = _inference(p, G, name, case, B, (1, B - 2))
    assert len(full) >= 4
    for (j, t), out in full.items():
        check_inference(G, name, j, t, out)
    small = _inference(p, G, name, case, 3, (2, 1))
    assert small.keys() == full.keys()
    for key, out in small.items():
        for x, y in zip(out, full[key]):
            np.testing.assert_array_equal(x, y, err_msg=str(key))
    p.close()


@pytest.mark.parametrize('case', FULL_CASES, ids=IDS)
def test_fullsize_search_in_batch_matches_reference(case):
    """The reference's recorded search at a middle row of a batch (C4: 128 envs, C5 / C5-19: 16), the other rows being the same position
    with other seeded draws: visits, policy and action equal to the fixture, root value within 1e-4."""
    name, A = case[0], case[3]
    G = load(name)
    g = f'{name}_search'
    kw = search_kwargs(G, name)
    S, B = kw['num_simulations'], SEARCH_ENVS[name]
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
    assert len({tuple(v) for v in r['visits']}) > 1  # other draws search differently: the fixture row is not matched by accident of layout
    p.close()


def test_fullsize_inference_on_generic_builds():
    """The same inference tests with MZ_CONV_SPEC=0 (no shape-specialised build: nine ragged 8 x 8 tiles per 19 x 19 image, the generic
    whole-image and tiled kernels elsewhere), so the fallback geometry is pinned to the reference too.  The switch is read once per
    process: child pytest."""
    env = dict(os.environ, MZ_CONV_SPEC='0')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k', 'inference_in_batch'], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert '3 passed' in r.stdout, r.stdout[-1000:]
