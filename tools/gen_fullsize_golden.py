#!/usr/bin/env python3
"""Reference fixtures for the full-size conv nets: tests/golden/fullsize_c4.npz, fullsize_c5.npz, fullsize_c5_19.npz.

Runs the REFERENCE implementation (imported read-only through oracle/_refshim.py, as oracle/gen_golden.py does) on the three seeded
128-plane x 8-block nets of tests/fullsize_cases.py and records inputs, the random draws the reference consumed, its outputs and the
yardsticks below -- never weights (the tests rebuild them from the seed with tests/helpers.seeded_state_dict) and no reference source.

Per net:
  inference  two observations (boards: one of `rand < 0.3` planes, one Gomoku position a few moves in; Atari: frames of integers 0..255),
             each with initial_inference and two chained recurrent_inference steps.  Observations are stored as uint8 (tests cast).  If a
             file would exceed the size limit for a committed file (1 MiB), the second observation's recurrent chain of that net is left
             out (`<net>_1_actions` is then empty); today all three fit with both chains (c5_19, 185 KB per hidden state: 0.73 MiB).
  yardstick  the same seeded net in float64 (a .double() copy, same code path) on the same inputs -- every recurrent step fed the
             float32 reference's previous hidden state, as the tests feed it -- and, per output kind,
                 <net>_e32_<kind> = max |reference float32 - reference float64|     over everything recorded for that net
             for kind in init_hidden, init_pi, init_value, rec_hidden, rec_pi, rec_value, rec_reward.  The tests derive their absolute
             tolerances from these (tests/test_oracle_fullsize.py), never from the oracle's or the kernels' outputs.  The float64
             priors themselves are stored too (`<net>_<j>_init_pi_f64`, `_rec_pi_f64`): where 4 * e32 exceeds 100 x the toy-size bar
             (C5's initial prior), the float32 record is no usable yardstick and the tests compare with the float64 one.
  search     one reference uct_search with its draws recorded, temperature 1, not deterministic, at the BASELINE settings of the net
             (tests/fullsize_cases.py: FIXTURE_SIMS simulations).  Each candidate seed is searched twice from the same np.random.seed,
             with the float32 net and with the float64 net behind a wrapper that casts inputs and outputs; a seed is kept only if both
             runs give the same visit vector, the same number of recorded tie-breaks, the same action, and root values within 1e-6 --
             so that the recorded visit counts do not hang on a rounding coin-flip of the reference itself.  Seeds are tried in a fixed
             order, at most 20; the number tried is stored as <net>_search_seeds_tried.
             Root values within 1e-6 is out of reach where one float32 evaluation of the reference is itself further than that from
             its float64 twin: C4's categorical value head gives |v| of several hundred with these weights (one float32 ulp there is
             6e-5, and the reference's float32 signed_parabolic cancels: e32 of a value is 2.8e-3) -- on all 20 seeds visits,
             tie-breaks and action agree and the root values are 1.0e-3..3.4e-3 apart.  The cause is per evaluation, so fewer
             simulations would not change it and C4's simulation count is not halved.  Only if no seed in 20 meets 1e-6, the first
             seed is kept whose root values are within 4 * (e32 value + e32 reward) of the net's own yardsticks; the bar used and the
             float64 root value are stored as <net>_search_root_value_agree_tol / _root_value_f64.  Today: c5 1e-6 (17th seed), c5_19
             1e-6 (9th seed; the board nets' values sit a steady 4e-6 / 1e-5 from their float64 twins, so most seeds miss it while
             agreeing on everything else), c4 1.3e-2 at |v| = 867 (first seed, root values 2.3e-3 apart: 2.6e-6 of |v|, against the
             1e-4 * |v| the tests allow).

Deterministic: two runs give identical arrays.  Build container only (it needs the reference checkout); takes about ten minutes of one core:

    python tools/gen_fullsize_golden.py            # all three nets
    python tools/gen_fullsize_golden.py c5_19      # selected nets
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'oracle'))
sys.path.insert(0, os.path.join(REPO, 'tests'))

import gen_golden as gg  # noqa: E402  (installs the reference shim)
import torch  # noqa: E402
from fullsize_cases import FIXTURE_SIMS, FULL, FULL_CASES  # noqa: E402

SIZE_LIMIT = 1 << 20
MAX_SEEDS = 20
KINDS = ('init_hidden', 'init_pi', 'init_value', 'rec_hidden', 'rec_pi', 'rec_value', 'rec_reward')


class Net64:
    """The float64 copy of a reference net behind the two inference methods uct_search calls: float32 tensors in, and out what the
    float32 net hands back -- float32 arrays for hidden state and prior, Python floats for value and reward."""

    def __init__(self, net):
        self.net = copy.deepcopy(net).double()
        self.net.eval()

    def _cast(self, o):
        return gg.ref_network.NetworkOutputs(hidden_state=o.hidden_state.astype(np.float32), reward=o.reward,
                                             pi_probs=o.pi_probs.astype(np.float32), value=o.value)

    def initial_inference(self, x):
        return self._cast(self.net.initial_inference(x.double()))

    def recurrent_inference(self, hidden_state, action):
        return self._cast(self.net.recurrent_inference(hidden_state.double(), action))


def _as_uint8(obs):
    u = np.asarray(obs).astype(np.uint8)
    assert np.array_equal(u.astype(np.float64), np.asarray(obs, np.float64))
    return u


def _gomoku_position(rng, N, moves):
    env = gg.GomokuEnv(board_size=N, stack_history=4)
    obs = env.reset()
    for _ in range(moves):
        legal = np.where(env.actions_mask[:N * N])[0]
        obs, _, done, _ = env.step(int(rng.choice(legal)))
        assert not done
    return _as_uint8(obs), env.actions_mask.copy(), (env.current_player, env.opponent_player)


def _e32(net64, prefix, out, e):
    """Fold |float32 record - float64 evaluation| of one recorded inference case into the running maxima `e`."""
    def upd(kind, a32, a64):
        e[kind] = max(e[kind], float(np.max(np.abs(np.asarray(a32, np.float64) - np.asarray(a64, np.float64)))))

    obs = torch.from_numpy(out[f'{prefix}_obs']).to(torch.float64)[None]
    o = net64.initial_inference(obs)
    upd('init_hidden', out[f'{prefix}_init_hidden'], o.hidden_state)
    upd('init_pi', out[f'{prefix}_init_pi'], o.pi_probs)
    out[f'{prefix}_init_pi_f64'] = np.asarray(o.pi_probs, np.float64)
    pis = []
    upd('init_value', out[f'{prefix}_init_value'], o.value)
    for t, a in enumerate(out[f'{prefix}_actions']):
        h_in = out[f'{prefix}_init_hidden'] if t == 0 else out[f'{prefix}_rec_hidden'][t - 1]
        o = net64.recurrent_inference(torch.from_numpy(h_in).to(torch.float64)[None], torch.tensor([[int(a)]], dtype=torch.long))
        upd('rec_hidden', out[f'{prefix}_rec_hidden'][t], o.hidden_state)
        upd('rec_pi', out[f'{prefix}_rec_pi'][t], o.pi_probs)
        upd('rec_value', out[f'{prefix}_rec_value'][t], o.value)
        upd('rec_reward', out[f'{prefix}_rec_reward'][t], o.reward)
        pis.append(np.asarray(o.pi_probs, np.float64))
    if pis:
        out[f'{prefix}_rec_pi_f64'] = np.stack(pis)


def gen_inference(name, net, net64, second_chain):
    case = FULL[name][0]
    kind, ishape, A, N = case[1], case[2], case[3], case[2][1]
    rng = np.random.RandomState(6000 + FULL_CASES.index(case))
    out, e = {}, dict.fromkeys(KINDS, 0.0)
    for j in range(2):
        if kind == 'atari':
            obs = rng.randint(0, 256, size=ishape).astype(np.uint8)
        elif j == 0:
            obs = (rng.rand(*ishape) < 0.3).astype(np.uint8)
        else:
            obs = _gomoku_position(rng, N, 7)[0]
        actions = rng.randint(0, A, size=2)
        p = f'{name}_{j}'
        gg._infer_case(net, obs, actions, p, out)
        if j == 1 and not second_chain:
            for k in ('rec_hidden', 'rec_reward', 'rec_value', 'rec_pi'):
                del out[f'{p}_{k}']
            out[f'{p}_actions'] = np.zeros((0,), np.int32)
        _e32(net64.net, p, out, e)
    for k, v in e.items():
        out[f'{name}_e32_{k}'] = np.float64(v)
    return out


def root_value_bar(name, inf):
    """The fallback bar on |root value float32 - root value float64| (module docstring): four times the reference's own float32 error of
    one value plus one reward evaluation, from the net's measured yardsticks."""
    e = max(float(inf[f'{name}_e32_init_value']), float(inf[f'{name}_e32_rec_value'])) + float(inf[f'{name}_e32_rec_reward'])
    return max(1e-6, 4.0 * e)


def gen_search(name, net, net64, fallback_bar):
    case, _, _, kw = FULL[name]
    kind, ishape, A, N = case[1], case[2], case[3], case[2][1]
    k = FULL_CASES.index(case)
    rng = np.random.RandomState(7000 + k)
    board = kind == 'board'
    cfg = gg.make_config(kw['discount'], kw['root_dirichlet_alpha'], FIXTURE_SIMS[name], board, kw.get('known_bounds'), case[6], case[7])
    if board:
        obs, mask, players = _gomoku_position(rng, N, 6)
    else:
        obs, mask, players = rng.randint(0, 256, size=ishape).astype(np.uint8), np.ones(A, bool), (1, 1)
    p = f'{name}_search'
    runs = []
    for i in range(MAX_SEEDS):
        seed = 4100 + 100 * k + i
        r32, r64 = {}, {}
        gg._search_case(net, cfg, obs, mask, players, 1.0, False, seed, p, r32, A)
        gg._search_case(net64, cfg, obs, mask, players, 1.0, False, seed, p, r64, A)
        same = (np.array_equal(r32[f'{p}_visits'], r64[f'{p}_visits']) and int(r32[f'{p}_n_tie']) == int(r64[f'{p}_n_tie'])
                and int(r32[f'{p}_out_action']) == int(r64[f'{p}_out_action']))
        gap = abs(float(r32[f'{p}_out_root_value']) - float(r64[f'{p}_out_root_value']))
        print(f'  {name}: seed {seed}: float32 and float64 searches: visits, ties and action {"agree" if same else "differ"}, '
              f'root values {gap:.3e} apart', flush=True)
        runs.append((same, gap, r32, r64))
        if same and gap <= 1e-6:
            break
    for bar in (1e-6, fallback_bar):
        for i, (same, gap, r32, r64) in enumerate(runs):
            if same and gap <= bar:
                out = {f'{p}_{key}': v for key, v in gg.cfg_arrays(cfg).items()}
                out.update(r32)
                out[f'{p}_seeds_tried'] = np.int32(i + 1)
                out[f'{p}_root_value_f64'] = r64[f'{p}_out_root_value']
                out[f'{p}_root_value_agree_tol'] = np.float64(bar)
                return out
    raise SystemExit(f'{name}: no seed in {MAX_SEEDS} on which the float32 and float64 reference searches agree')


def main(names):
    for name in names:
        net = gg.build_conv(FULL[name][0])
        net64 = Net64(net)
        full = gen_inference(name, net, net64, True)
        search = gen_search(name, net, net64, root_value_bar(name, full))
        path = os.path.join(REPO, 'tests', 'golden', f'fullsize_{name}.npz')
        for second_chain in (True, False):
            out = full if second_chain else gen_inference(name, net, net64, False)
            out.update(search)
            np.savez_compressed(path, **out)
            if os.path.getsize(path) <= SIZE_LIMIT:
                break
        assert os.path.getsize(path) <= SIZE_LIMIT, path
        print(path, len(out), 'arrays,', os.path.getsize(path), 'bytes, second recurrent chain:', second_chain)
        for kind in KINDS:
            print(f'  {name}_e32_{kind} = {float(out[f"{name}_e32_{kind}"]):.3e}')


if __name__ == '__main__':
    main(sys.argv[1:] or [c[0] for c in FULL_CASES])
