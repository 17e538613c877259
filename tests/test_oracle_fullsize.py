"""The oracle at the full sizes -- C4 (Atari, 8 x 96 x 96), C5 (Gomoku 15 x 15, 226 actions), C5-19 (19 x 19, 362 actions), each 128
planes x 8 residual blocks -- against the reference outputs recorded by tools/gen_fullsize_golden.py (tests/golden/fullsize_<net>.npz):
8 k-blocks x 9 taps per conv output, two 64-channel output slices, the folded BatchNorm of 128-channel layers, 33 convs of depth.

Tolerances.  rtol is that of tests/test_oracle_nets.py.  atol is, per net and output kind,

    atol = max(atol of test_oracle_nets.py, 4 * e32[kind]),     e32[kind] = max |reference float32 - reference float64|

where e32 is measured by the generator on the reference alone and stored in the fixture (`<net>_e32_<kind>`): the reference's float32
result and ours are each about e32 from the exact value in unrelated summation orders, hence up to about 2 * e32 apart, and a factor
two on top keeps an honest implementation from flaking.  A dropped k-block, a wrong tap or a mis-folded BatchNorm moves a normalised
hidden state by O(0.1).  No bar here was chosen by looking at the oracle's or the kernels' output.  Measured (this fixture set):

    kind          existing atol   e32 c4     e32 c5     e32 c5_19
    init_hidden   2e-6            4.112e-07  9.025e-07  1.020e-06
    init_pi       1e-7            3.058e-07  2.707e-06  7.990e-07
    init_value    2e-4            1.737e-04  9.081e-07  1.211e-05
    rec_hidden    2e-6            1.652e-06  9.272e-07  1.254e-06
    rec_pi        1e-7            2.270e-06  1.678e-06  1.423e-06
    rec_value     2e-4            2.752e-03  2.106e-06  1.593e-05
    rec_reward    2e-4            5.606e-04  2.578e-06  1.305e-05

(C4's values are several hundred with seeded weights, and the reference's float32 signed_parabolic cancels: util.py:27.)  For one
entry, C5's init_pi, 4 * e32 = 1.08e-5 is above 100 x the existing bar (1e-5): the float32 record is then no usable absolute yardstick,
and that output is compared with the reference's float64 record, which the fixture keeps for the priors, at atol = max(existing,
2 * e32) -- our float32 result is about e32 from it, as the reference's own is.

Searches: the generator keeps a (position, seed) only if the reference's float32 and float64 searches agree on visits, number of
tie-breaks and action, and on the root value within 1e-6 -- or, where a single float32 value of the reference is itself further than
that from its float64 twin (C4: |v| = 867, e32 2.8e-3), within 4 * (e32 value + e32 reward); tools/gen_fullsize_golden.py has the
figures.  Seeds tried: c5 17 and c5_19 9 (at 1e-6); c4 20 at 1e-6, then the first seed at the e32-derived bar.  So the demands of the
toy fixtures hold here too: visits, policy and action equal, root value within 1e-4 * max(1, |v|).

The scalar oracle needs 1.8 s per Gomoku simulation at 15 x 15 and 2.9 s at 19 x 19: the C5 search (200 simulations, 350 s) is most of
this file's wall time, and C5-19's recorded search has 20 simulations to keep the file under 8 minutes;
MZ_FAST_TESTS=1 drops that one case, as it drops the 200-simulation spot check of tests/test_gpu_conv.py."""
import os

import numpy as np
import pytest

from fullsize_cases import FULL_CASES
from helpers import build_conv, load_golden
from test_oracle_nets import HID_TOL, PI_TOL, VAL_TOL

IDS = [c[0] for c in FULL_CASES]
BASE_TOL = dict(init_hidden=HID_TOL, init_pi=PI_TOL, init_value=VAL_TOL, rec_hidden=HID_TOL, rec_pi=PI_TOL, rec_value=VAL_TOL,
                rec_reward=VAL_TOL)


def load(name):
    return load_golden(f'fullsize_{name}.npz')


def usable(G, name, kind):
    """4 * e32 above 100 x the existing bar means that the float32 reference is no usable yardstick for that output."""
    return 4.0 * float(G[f'{name}_e32_{kind}']) <= 100.0 * BASE_TOL[kind]['atol']


def tol(G, name, kind):
    """rtol of the toy-size tests; atol = max(theirs, 4 * e32[kind]) with e32 from the fixture, against the float32 record.  Where that is
    no usable yardstick, the comparison is with the reference's float64 record instead (kept for the priors): our float32 result is about
    e32 from it, as the reference's own is, hence atol = max(theirs, 2 * e32[kind])."""
    base = BASE_TOL[kind]
    e32 = float(G[f'{name}_e32_{kind}'])
    return dict(rtol=base['rtol'], atol=max(base['atol'], (4.0 if usable(G, name, kind) else 2.0) * e32))


def record(G, name, j, kind):
    """The reference's record of one output kind of observation j: float32, or float64 where the float32 one is no usable yardstick."""
    if usable(G, name, kind):
        return G[f'{name}_{j}_{kind}']
    assert kind in ('init_pi', 'rec_pi'), (name, kind, float(G[f'{name}_e32_{kind}']))  # hidden, value, reward: no float64 record is kept
    return G[f'{name}_{j}_{kind}_f64']


def check_inference(G, name, j, step, outputs):
    """One inference result (hidden, reward, pi, value as flat arrays / scalars) of fixture observation j against the reference: step -1 is
    the initial inference, step t >= 0 the t-th recurrent one."""
    h, r, pi, v = outputs
    if step < 0:
        np.testing.assert_allclose(h, record(G, name, j, 'init_hidden').reshape(-1), **tol(G, name, 'init_hidden'))
        np.testing.assert_allclose(pi, record(G, name, j, 'init_pi'), **tol(G, name, 'init_pi'))
        np.testing.assert_allclose(v, record(G, name, j, 'init_value'), **tol(G, name, 'init_value'))
        assert float(G[f'{name}_{j}_init_reward']) == 0.0
    else:
        np.testing.assert_allclose(h, record(G, name, j, 'rec_hidden')[step].reshape(-1), **tol(G, name, 'rec_hidden'))
        np.testing.assert_allclose(r, record(G, name, j, 'rec_reward')[step], **tol(G, name, 'rec_reward'))
        np.testing.assert_allclose(v, record(G, name, j, 'rec_value')[step], **tol(G, name, 'rec_value'))
        np.testing.assert_allclose(pi, record(G, name, j, 'rec_pi')[step], **tol(G, name, 'rec_pi'))


def hidden_in(G, name, j, step):
    """The reference's hidden state that goes into recurrent step `step` of observation j."""
    p = f'{name}_{j}'
    return (G[f'{p}_init_hidden'] if step == 0 else G[f'{p}_rec_hidden'][step - 1]).reshape(-1)


def check_search(G, name, visits, pi, action, root_value):
    p = f'{name}_search'
    np.testing.assert_array_equal(visits, G[f'{p}_visits'])
    np.testing.assert_array_equal(pi, G[f'{p}_out_pi'])
    assert action == int(G[f'{p}_out_action'])
    rv = float(G[f'{p}_out_root_value'])
    assert abs(root_value - rv) <= 1e-4 * max(1.0, abs(rv))


def search_kwargs(G, name):
    p = f'{name}_search'
    return dict(num_simulations=int(G[f'{p}_sims']), discount=float(G[f'{p}_discount']), is_board_game=bool(G[f'{p}_board']),
                known_bounds=(float(G[f'{p}_kb_min']), float(G[f'{p}_kb_max'])) if int(G[f'{p}_has_bounds']) else None,
                root_dirichlet_alpha=float(G[f'{p}_alpha']), root_exploration_eps=float(G[f'{p}_eps']), pb_c_base=float(G[f'{p}_pb_c_base']),
                pb_c_init=float(G[f'{p}_pb_c_init']))


@pytest.mark.parametrize('case', FULL_CASES, ids=IDS)
def test_fullsize_inference_matches_reference(oracle, case):
    """Every initial and recurrent output at the bars of the module docstring, each recurrent step fed the reference's previous hidden
    state."""
    name = case[0]
    G = load(name)
    onet = oracle.Net.from_module(build_conv(case), 'conv')
    steps = 0
    for j in range(2):
        out = onet.initial_inference(G[f'{name}_{j}_obs'].astype(np.float32))
        assert out[2].shape == (case[3],)
        check_inference(G, name, j, -1, out)
        for t, a in enumerate(G[f'{name}_{j}_actions']):
            check_inference(G, name, j, t, onet.recurrent_inference(hidden_in(G, name, j, t), int(a)))
            steps += 1
    assert steps >= 2  # at least the first observation's chain is in every fixture


_SEARCH = [c for c in FULL_CASES if not (c[0] == 'c5' and os.environ.get('MZ_FAST_TESTS') == '1')]


@pytest.mark.parametrize('case', _SEARCH, ids=[c[0] for c in _SEARCH])
def test_fullsize_search_matches_reference(oracle, case):
    """The reference's uct_search at the BASELINE settings (C4: 50 simulations, alpha 0.25, discount 0.997, no bounds; C5: 200
    simulations, alpha 0.03, bounds (-1, 1), two players; C5-19: the same at 19 x 19 with 20 simulations) replayed with its recorded
    noise, tie-break and final-sample draws: visits, policy and action equal, root value within 1e-4."""
    name, A = case[0], case[3]
    G = load(name)
    p = f'{name}_search'
    kw = search_kwargs(G, name)
    assert int(G[f'{p}_has_noise']) and 1 <= int(G[f'{p}_seeds_tried']) <= 20
    onet = oracle.Net.from_module(build_conv(case), 'conv')
    cfg = oracle.make_config(A, kw['num_simulations'], kw['discount'], kw['is_board_game'], kw['known_bounds'], kw['root_dirichlet_alpha'],
                             kw['root_exploration_eps'], kw['pb_c_base'], kw['pb_c_init'])
    r = oracle.uct_search(cfg, onet, G[f'{p}_obs'].astype(np.float32), G[f'{p}_mask'], int(G[f'{p}_cur_player']), int(G[f'{p}_opp_player']),
                          float(G[f'{p}_temperature']), bool(G[f'{p}_deterministic']), noise=G[f'{p}_noise'], u_tie=G[f'{p}_u_tie'],
                          u_final=float(G[f'{p}_u_final']))
    check_search(G, name, r['visits'], r['pi'], r['action'], r['root_value'])
