"""The oracle above 256 actions: 19 x 19 (362 actions) and 16 x 16 (257 actions) board nets against the reference outputs recorded
by tools/gen_board_golden.py (tests/golden/board19_cases.npz), at the tolerances of test_oracle_nets.py / test_oracle_search.py."""
import numpy as np
import pytest

from board19_cases import BOARD_CASES
from helpers import build_conv, load_golden
from test_oracle_nets import HID_TOL, PI_TOL, VAL_TOL

G = load_golden('board19_cases.npz')
IDS = [c[0] for c in BOARD_CASES]


@pytest.mark.parametrize('case', BOARD_CASES, ids=IDS)
def test_board_inference_matches_reference(oracle, case):
    onet = oracle.Net.from_module(build_conv(case), 'conv')
    for j in range(2):
        p = f'{case[0]}_{j}'
        h, r0, pi, v = onet.initial_inference(G[f'{p}_obs'])
        assert pi.shape == (case[3],)
        np.testing.assert_allclose(h, G[f'{p}_init_hidden'].reshape(-1), **HID_TOL)
        np.testing.assert_allclose(pi, G[f'{p}_init_pi'], **PI_TOL)
        np.testing.assert_allclose(v, G[f'{p}_init_value'], **VAL_TOL)
        for t, a in enumerate(G[f'{p}_actions']):
            h_in = G[f'{p}_init_hidden'] if t == 0 else G[f'{p}_rec_hidden'][t - 1]
            h, r, pi, v = onet.recurrent_inference(h_in, int(a))
            np.testing.assert_allclose(h, G[f'{p}_rec_hidden'][t].reshape(-1), **HID_TOL)
            np.testing.assert_allclose(r, G[f'{p}_rec_reward'][t], **VAL_TOL)
            np.testing.assert_allclose(v, G[f'{p}_rec_value'][t], **VAL_TOL)
            np.testing.assert_allclose(pi, G[f'{p}_rec_pi'][t], **PI_TOL)


def search_config(oracle, name, A):
    g = f'{name}_search'
    return oracle.make_config(A, int(G[f'{g}_sims']), float(G[f'{g}_discount']), bool(G[f'{g}_board']),
                              (float(G[f'{g}_kb_min']), float(G[f'{g}_kb_max'])), float(G[f'{g}_alpha']), float(G[f'{g}_eps']),
                              float(G[f'{g}_pb_c_base']), float(G[f'{g}_pb_c_init']))


@pytest.mark.parametrize('case', BOARD_CASES, ids=IDS)
def test_board_search_matches_reference(oracle, case):
    """Root prior over 362 / 257 actions (Dirichlet alpha 0.03), pairwise sums past 256 elements, visits, policy and action."""
    name, A = case[0], case[3]
    onet = oracle.Net.from_module(build_conv(case), 'conv')
    p = f'{name}_search'
    assert int(G[f'{p}_has_noise'])
    r = oracle.uct_search(search_config(oracle, name, A), onet, G[f'{p}_obs'], G[f'{p}_mask'], int(G[f'{p}_cur_player']),
                          int(G[f'{p}_opp_player']), float(G[f'{p}_temperature']), bool(G[f'{p}_deterministic']), noise=G[f'{p}_noise'],
                          u_tie=G[f'{p}_u_tie'], u_final=float(G[f'{p}_u_final']))
    np.testing.assert_array_equal(r['visits'], G[f'{p}_visits'])
    np.testing.assert_array_equal(r['pi'], G[f'{p}_out_pi'])
    assert r['action'] == int(G[f'{p}_out_action'])
    rv = float(G[f'{p}_out_root_value'])
    assert abs(r['root_value'] - rv) <= 1e-4 * max(1.0, abs(rv))
