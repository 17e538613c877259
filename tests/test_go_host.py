"""Go on the host (no GPU): `games.GoEnv` -- the definition of the device env MZ_ENV_GO -- on the hand-written scripted games of
go_cases.py; a second implementation written independently of it (sets of points, one stack flood fill per group, no propagation) and
the numpy model of the device kernel's formulation, all three ply by ply on random games; the published counts of legal positions;
the model's planted mistakes; the declarations."""
import os
import re

import numpy as np
import pytest

import go_cases as gc
from helpers import REPO
from muzero_amd.games import GoEnv


# ---------------------------------------------------------------------------------------------------------
# the second implementation: sets and flood fill
# ---------------------------------------------------------------------------------------------------------
class SetGo:
    """Go with GoEnv's interface, from the rules' text: stones are two sets of points, a group is found by a stack flood fill, its
    liberties are a set; legality of a point is judged from the sets of the groups around it."""

    def __init__(self, rows, cols, komi2=15, max_plies=0, allow_resign=True, stack_history=4):
        self.rows, self.cols, self.nn = rows, cols, rows * cols
        self.komi2, self.max_plies, self.allow_resign, self.stack_history = komi2, max_plies or 2 * rows * cols, allow_resign, stack_history
        self.adj = {(r, c): [(r + dr, c + dc) for dr, dc in ((0, 1), (0, -1), (1, 0), (-1, 0)) if 0 <= r + dr < rows and 0 <= c + dc < cols]
                    for r in range(rows) for c in range(cols)}
        self.stones = {1: set(), 2: set()}
        self.current_player, self.steps, self.winner, self.over = 1, 0, None, False
        self.forbidden, self.passes = None, 0
        self.past = []  # (black set, white set) after every ply
        self._mask()

    def group(self, stones, p):
        colour = 1 if p in stones[1] else 2
        g, libs, stack = {p}, set(), [p]
        while stack:
            for q in self.adj[stack.pop()]:
                if q in stones[colour]:
                    if q not in g:
                        g.add(q)
                        stack.append(q)
                elif q not in stones[3 - colour]:
                    libs.add(q)
        return g, libs

    def groups_ok(self, stones) -> bool:
        return all(self.group(stones, p)[1] for colour in (1, 2) for p in stones[colour])

    def _mask(self):
        me, you = self.current_player, 3 - self.current_player
        m = np.zeros(self.nn + 2, np.bool_)
        info = {}
        for colour in (1, 2):
            for p in self.stones[colour]:
                if p not in info:
                    g, libs = self.group(self.stones, p)
                    for s in g:
                        info[s] = libs
        for p in self.adj:
            if p in info or p == self.forbidden:
                continue
            ok = False
            for q in self.adj[p]:
                if q not in info:
                    ok = True  # an empty point beside it
                elif q in self.stones[me] and info[q] - {p}:
                    ok = True  # a friend with a liberty elsewhere
                elif q in self.stones[you] and info[q] == {p}:
                    ok = True  # it takes the last liberty of an opposing group
            m[p[0] * self.cols + p[1]] = ok
        m[self.nn] = True
        m[self.nn + 1] = self.allow_resign
        self.actions_mask = m

    @property
    def board(self):
        b = np.zeros((self.rows, self.cols), np.int8)
        for colour in (1, 2):
            for p in self.stones[colour]:
                b[p] = colour
        return b

    def score(self):
        area = {1: len(self.stones[1]), 2: len(self.stones[2])}
        seen = set()
        for p in self.adj:
            if p in seen or p in self.stones[1] or p in self.stones[2]:
                continue
            region, borders, stack = {p}, set(), [p]
            while stack:
                for q in self.adj[stack.pop()]:
                    if q in self.stones[1]:
                        borders.add(1)
                    elif q in self.stones[2]:
                        borders.add(2)
                    elif q not in region:
                        region.add(q)
                        stack.append(q)
            seen |= region
            if borders == {1}:
                area[1] += len(region)
            if borders == {2}:
                area[2] += len(region)
        return area[1], area[2]

    def step(self, action):
        assert not self.over and self.actions_mask[action]
        me, you = self.current_player, 3 - self.current_player
        reward, self.forbidden = 0.0, None
        if action == self.nn + 1:
            reward, self.winner, self.over = -1.0, you, True
        else:
            if action == self.nn:
                self.passes += 1
            else:
                self.passes = 0
                p = divmod(action, self.cols)
                self.stones[me].add(p)
                taken = set()
                for q in self.adj[p]:
                    if q in self.stones[you] and q not in taken:
                        g, libs = self.group(self.stones, q)
                        if not libs:
                            taken |= g
                self.stones[you] -= taken
                g, libs = self.group(self.stones, p)
                assert libs, 'suicide'
                if len(taken) == 1 and len(g) == 1 and len(libs) == 1:
                    (self.forbidden,) = taken
            self.past.append((frozenset(self.stones[1]), frozenset(self.stones[2])))
            if self.passes == 2 or self.steps + 1 == self.max_plies:
                self.over = True
                black, white = self.score()
                if 2 * black != 2 * white + self.komi2:
                    self.winner = 1 if 2 * black > 2 * white + self.komi2 else 2
                    reward = 1.0 if self.winner == me else -1.0
        if not self.over:
            self.current_player = you
            self._mask()
        self.steps += 1
        return self.observation(), reward, self.over, {}

    def observation(self):
        me = self.current_player
        out = np.zeros((2 * self.stack_history + 1, self.rows, self.cols), np.int8)
        for k in range(self.stack_history):
            if k < len(self.past):
                for j, colour in enumerate((me, 3 - me)):
                    for p in self.past[-1 - k][colour - 1]:
                        out[2 * k + j][p] = 1
        out[-1] = 1 if me == 1 else 0
        return out


def make(kind, c, stack_history=4, mistake=None):
    kw = dict(c['rules'], stack_history=stack_history)
    if kind == 'env':
        return GoEnv(c['rows'], c['cols'], **kw)
    if kind == 'sets':
        return SetGo(c['rows'], c['cols'], **kw)
    return gc.GoModel(c['rows'], c['cols'], mistake=mistake, **kw)


KO_OF = {'env': lambda e: e.ko_point, 'sets': lambda e: None if e.forbidden is None else e.forbidden[0] * e.cols + e.forbidden[1],
         'model': lambda e: None if e.ko < 0 else e.ko}


# ---------------------------------------------------------------------------------------------------------
# scripted games
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stack_history', [1, 4])
@pytest.mark.parametrize('name', [c['name'] for c in gc.ALL_CASES])
def test_scripted_games_on_the_host_env(name, stack_history):
    c = gc.BY_NAME[name]
    gc.run_case(c, make('env', c, stack_history), KO_OF['env'])


@pytest.mark.parametrize('kind', ['sets', 'model'])
def test_scripted_games_on_the_other_two_implementations(kind):
    for c in gc.ALL_CASES:
        if c['name'] == 'spiral_19x19' and kind == 'sets':
            continue  # (398 plies with flood fills of up to 199 stones: the 9 x 9 spiral asks the same of it)
        gc.run_case(c, make(kind, c), KO_OF[kind])


def test_the_cases_are_what_their_names_say():
    """Boards-only checks of the hand-written positions: what is captured where, and that the list holds every required case."""
    names = {c['name'] for c in gc.ALL_CASES}
    assert {'capture_centre', 'capture_edge', 'capture_corner', 'capture_group', 'capture_two_groups', 'capture_two_stones_no_ko',
            'ko_retake_illegal', 'ko_retake_after_ply', 'ko_cleared_by_pass', 'snapback', 'edge_wrap_5x5', 'edge_wrap_4x6', 'spiral_9x9',
            'spiral_19x19', 'end_two_passes_empty', 'end_max_plies', 'end_resign', 'end_no_resign', 'count_neutral_draw',
            'count_empty_draw', 'count_seki', 'count_seki_draw', 'final_pass_loses'} <= names
    assert set(gc.MISTAKES.values()) <= names

    def removed(c, ply):  # stones of the side not moving that the ply takes off
        before = gc.parse(c['plies'][ply - 2][1]) if ply > 1 else np.zeros((c['rows'], c['cols']), np.int8)
        after = gc.parse(c['plies'][ply - 1][1])
        return int(np.count_nonzero((before != 0) & (after == 0)))

    for name, ply, n in (('capture_centre', 7, 1), ('capture_edge', 5, 1), ('capture_corner', 3, 1), ('capture_group', 5, 2),
                         ('capture_two_groups', 7, 2), ('capture_two_stones_no_ko', 7, 2), ('ko_retake_illegal', 9, 1), ('snapback', 13, 1),
                         ('snapback', 14, 5), ('edge_wrap_5x5', 4, 1), ('edge_wrap_5x5', 10, 1), ('edge_wrap_4x6', 4, 1), ('edge_wrap_4x6', 10, 1)):
        assert removed(gc.BY_NAME[name], ply) == n, (name, ply)
    for c in gc.ALL_CASES:  # a ply adds at most the mover's stone and removes only the other colour's
        prev = np.zeros((c['rows'], c['cols']), np.int8)
        for i, ply in enumerate(c['plies']):
            b, mover = gc.parse(ply[1]), 1 + i % 2
            assert b.shape == (c['rows'], c['cols'])
            if isinstance(ply[0], tuple):
                assert prev[ply[0]] == 0 and b[ply[0]] == mover, (c['name'], i + 1)
                assert np.count_nonzero(b == mover) == np.count_nonzero(prev == mover) + 1
            else:
                assert np.array_equal(b, prev), (c['name'], i + 1)
            assert not ((prev == mover) & (b != mover)).any(), (c['name'], i + 1)
            prev = b
    for name, n, stones in (('spiral_9x9', 9, 49), ('spiral_19x19', 19, 199)):
        c = gc.BY_NAME[name]
        assert c['rows'] == n and removed(c, len(c['plies'])) == stones and len(c['plies']) == 2 * stones
    # the spirals' plies are read off the final patterns: two positions of each on the way, written out by hand, anchor the order
    for name, ply, board in (
            ('spiral_9x9', 20, 'XXXXXXXXX/OOOOOOOOX/.......O./.......O./........./........./........./........./.........'),
            ('spiral_9x9', 62, 'XXXXXXXXX/OOOOOOOOX/X......OX/XOOOOO.OX/XO...O.OX/XO..OO.OX/XO.....OX/XOOOOOOOX/XXXXXXXXX'),
            ('spiral_19x19', 40, '/'.join(['X' * 19, 'O' * 18 + 'X', '.' * 17 + 'O.', '.' * 17 + 'O.'] + ['.' * 19] * 15)),
            ('spiral_19x19', 142, '/'.join(['X' * 19, 'O' * 18 + 'X', 'X' + '.' * 16 + 'OX', 'X' + 'O' * 8 + '.' * 8 + 'OX'] + ['XO' + '.' * 15 + 'OX'] * 13
                                           + ['X' + 'O' * 17 + 'X', 'X' * 19]))):
        assert gc.BY_NAME[name]['plies'][ply - 1][1] == board, (name, ply)
    # the edge-wrap stones are index neighbours and no board neighbours
    assert (0 * 5 + 4) + 1 == 1 * 5 + 0 and (2 * 6 + 5) + 1 == 3 * 6 + 0


def test_illegal_actions_raise_and_arguments_are_checked():
    e = GoEnv(5, 5)
    e.step(12)
    with pytest.raises(ValueError):
        e.step(12)
    with pytest.raises(ValueError):
        e.step(27)
    e = GoEnv(5, 5, allow_resign=False)
    with pytest.raises(ValueError):
        e.step(26)
    for bad in (dict(rows=2), dict(cols=20), dict(komi2=-1), dict(komi2=163), dict(max_plies=-1), dict(max_plies=163), dict(stack_history=0)):
        with pytest.raises(ValueError):
            GoEnv(**bad)
    e = GoEnv(3, 4, max_plies=24)
    assert e.num_actions == 14 and e.observation_shape == (9, 3, 4) and e.max_plies == 24 and GoEnv(3, 4).max_plies == 24
    e.step(12)
    _, r, done, _ = e.step(12)
    assert done and r == 1.0 and e.winner == 2
    with pytest.raises(RuntimeError):
        e.step(0)


# ---------------------------------------------------------------------------------------------------------
# three implementations, ply by ply, on random games
# ---------------------------------------------------------------------------------------------------------
# 5 x 5 and 4 x 6: 2 000 games each.  9 x 9: 60 and 19 x 19: 3 -- a ply of the definition costs a trial placement per enclosed empty point
# and the flood-fill implementation a fill per group, so a 19 x 19 game of up to 722 plies costs about what 300 games on 5 x 5 do; the
# large boards are here for the index arithmetic past 64 and 256 points, which a few long games cover, not for more positions.
RANDOM_GAMES = [(5, 5, 2000), (4, 6, 2000), (9, 9, 60), (19, 19, 3)]


@pytest.mark.parametrize('rows,cols,games', RANDOM_GAMES)
def test_three_implementations_agree_on_random_games(rows, cols, games):
    rs = np.random.RandomState(1000 * rows + cols)
    nn = rows * cols
    plies = ends = captures = kos = 0
    for g in range(games):
        rules = dict(komi2=int(rs.randint(0, 2 * nn + 1)) if g % 2 else 15, max_plies=int(rs.randint(1, 2 * nn + 1)) if g % 3 == 0 else 0,
                     allow_resign=bool(g % 4))
        env, sets, model = GoEnv(rows, cols, **rules), SetGo(rows, cols, **rules), gc.GoModel(rows, cols, **rules)
        done = False
        while not done:
            m = env.actions_mask
            assert np.array_equal(m, sets.actions_mask) and np.array_equal(m, model.actions_mask), (g, env.steps)
            legal = np.flatnonzero(m[:nn + 1])
            # mostly placements (a uniformly drawn pass ends games early); a resignation now and then where it is allowed
            u = rs.rand()
            a = nn + 1 if (u < 0.002 and m[nn + 1]) else nn if (u < 0.05 or len(legal) == 1) else int(legal[rs.randint(len(legal) - 1)])
            stones = np.count_nonzero(env.board)
            out = [x.step(a) for x in (env, sets, model)]
            captures += np.count_nonzero(env.board) < stones + (a < nn)
            kos += env.ko_point is not None
            for o in out[1:]:
                assert np.array_equal(out[0][0], o[0]) and out[0][1:3] == o[1:3], (g, env.steps, a)
            assert np.array_equal(env.board, sets.board) and np.array_equal(env.board, model.board), (g, env.steps, a)
            assert env.winner == sets.winner == model.winner and env.current_player == sets.current_player == model.current_player
            done = out[0][2]
            assert done or env.ko_point == KO_OF['sets'](sets) == KO_OF['model'](model)
            plies += 1
        ends += 1
    assert ends == games and captures > games // 2 and kos > 0, (plies, captures, kos)  # the games reach what the rules are about


# ---------------------------------------------------------------------------------------------------------
# the published numbers of legal positions
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols,count', [(2, 2, 57), (2, 3, 489), (3, 3, 12675)])
def test_legal_position_counts(rows, cols, count):
    """Every colouring of the board in which every group has a liberty: 57 on 2 x 2 and 12 675 on 3 x 3 are the published counts of legal
    Go positions (Tromp and Farneback); 489 on 2 x 3 by the same enumeration.  Each implementation's own liberty routine is asked."""
    nn = rows * cols
    model, sets = gc.GoModel(rows, cols), SetGo(rows, cols)
    found = [0, 0, 0]
    for code in range(3 ** nn):
        cells = np.array([(code // 3 ** i) % 3 for i in range(nn)], np.int8)
        board = cells.reshape(rows, cols)
        stones = {k: {(int(r), int(c)) for r, c in np.argwhere(board == k)} for k in (1, 2)}
        verdict = (GoEnv.all_groups_have_liberty(board), sets.groups_ok(stones), model.all_groups_have_liberty(cells))
        assert verdict[0] == verdict[1] == verdict[2], board
        for i in range(3):
            found[i] += verdict[i]
    assert found == [count] * 3


# ---------------------------------------------------------------------------------------------------------
# planted mistakes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mistake', sorted(gc.MISTAKES))
def test_every_planted_mistake_is_caught_by_its_named_case(mistake):
    c = gc.BY_NAME[gc.MISTAKES[mistake]]
    gc.run_case(c, make('model', c), KO_OF['model'])  # the model as it is passes
    with pytest.raises(AssertionError):
        gc.run_case(c, make('model', c, mistake=mistake), KO_OF['model'])


def test_uniformly_random_play_baseline():
    """The baseline of the learning numbers: tools/go_bench.py's `random` mode writes profiles/go/random_policy.json, and this
    recomputes it; only what is derivable is asserted besides."""
    import json
    import sys

    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import go_bench

    s = go_bench.random_policy_stats()
    assert abs(s['first_player_win'] + s['draw'] + s['first_player_loss'] - 1.0) < 1e-12 and s['draw'] == 0.0  # a half-integer komi
    assert 2 <= s['min_length'] <= s['mean_length'] <= s['max_length'] <= 2 * 49
    rec = json.load(open(os.path.join(REPO, 'profiles', 'go', 'random_policy.json')))
    assert set(rec) == set(s)
    for k, v in s.items():
        assert rec[k] == (pytest.approx(v, abs=1e-12) if isinstance(v, float) else v), k


# ---------------------------------------------------------------------------------------------------------
# declarations
# ---------------------------------------------------------------------------------------------------------
def test_config_names_and_constants():
    from muzero_amd import pipeline
    from muzero_amd import planner as pl
    from muzero_amd.config import make_go_config

    cfg = make_go_config()
    assert cfg.is_board_game and cfg.td_steps == 0 and cfg.discount == 1.0 and cfg.num_actions == 51 and cfg.input_shape == (9, 7, 7)
    assert (cfg.known_bounds.min, cfg.known_bounds.max) == (-1, 1)
    assert (cfg.komi2, cfg.max_plies, cfg.allow_resign) == (15, 0, False)
    assert make_go_config(rows=19, cols=19).num_actions == 363 and make_go_config(rows=4, cols=6).input_shape == (9, 4, 6)
    assert [cfg.visit_softmax_temperature_fn(s, 0) for s in (0, 7, 8, 40)] == [1.0, 1.0, 0.1, 0.1]
    assert pipeline.board_temperature_switch(cfg) == 8
    assert 'Go' in pipeline.DEVICE_ENVS and 'Go' in pipeline.ARENA_ENVS
    assert pipeline.resolve_self_play_envs('Go', 4) == ('device', 'Go')
    assert pipeline.resolve_self_play_envs(GoEnv(5, 5), 4) == ('device', 'Go')
    assert pipeline.resolve_arena_env('Go') == 'Go' and pipeline.resolve_arena_env(GoEnv(4, 6)) == 'Go'
    assert pipeline._go_args(GoEnv(5, 5, komi2=3, max_plies=20, allow_resign=False), cfg) == dict(komi2=3, max_plies=20, allow_resign=False)
    assert pipeline._go_args('Go', cfg) == dict(komi2=15, max_plies=0, allow_resign=False)
    assert pipeline._go_args('Go', object()) == dict(komi2=15, max_plies=0, allow_resign=True)
    header = open(os.path.join(REPO, 'include', 'mzplanner.h')).read()
    assert int(re.search(r'#define MZ_ENV_GO (\d+)', header).group(1)) == pl.ENV_GO == 10
    assert re.search(r'typedef struct \{\s*int32_t temp_switch_steps;[^}]*int32_t komi2;[^}]*int32_t max_plies;[^}]*int32_t allow_resign;[^}]*\} mz_go_env;', header)
    assert [f[0] for f in pl.MzGoEnv._fields_] == ['temp_switch_steps', 'komi2', 'max_plies', 'allow_resign']
    import ctypes

    from muzero_amd import build

    lib = ctypes.CDLL(build.build())
    for fn in ('mz_selfplay_reset_go', 'mz_go_debug_step', 'mz_go_debug_mask', 'mz_go_debug_board', 'mz_arena_reset_go'):
        assert re.search(r'^int ' + fn + r'\(', header, flags=re.M), fn  # an ordinary prototype
        assert hasattr(lib, fn), fn  # exported
        assert fn in pl.ABI_SYMBOLS and not any(ch.isdigit() for ch in fn)
    csrc = open(os.path.join(REPO, 'muzero_amd', 'csrc', 'mz_go.h')).read()
    assert re.search(r'constexpr int ENV_GO = 10;', csrc)
    assert '#include "mz_go.h"' in open(os.path.join(REPO, 'muzero_amd', 'csrc', 'planner.hip')).read()
