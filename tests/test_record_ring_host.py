"""CPU side of the compact record ring (include/mzplanner.h MZ_RECORD_FRAMES_U8): the window rule that rebuilds an observation from
one uint8 frame per move (tests/record_ring_cases.py) gives, row for row, what the project's own wrappers and encoder give; the data it is
checked on tells the likely mistakes apart; and the C declaration, the ctypes mirror and the Python switch agree."""
import os
import re

import numpy as np
import pytest

import record_ring_cases as rc
from helpers import REPO

CASES = [(n, s) for n in rc.GEOMETRIES for s in rc.SEEDS]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_data_has_the_hard_cases():
    for name, (C, H, W, S, A) in rc.GEOMETRIES.items():
        lens = []
        for seed in rc.SEEDS:
            d = rc.script(name, seed).done
            ends = np.flatnonzero(d)
            lens += list(np.diff(np.concatenate([[-1], ends])))
        assert 1 in lens and any(n < S for n in lens), name  # episodes of one move, episodes shorter than S
        assert S == 2 or any(1 < n < S for n in lens), name
        assert any(n > S for n in lens), name  # and full windows
    g = rc.GEOMETRIES
    assert any(c * h * w % 16 for c, h, w, _, _ in g.values()) and any(c * h * w % 16 == 0 for c, h, w, _, _ in g.values())
    assert any(c > 1 for c, *_ in g.values()) and any(a == 256 for *_, a in g.values())
    sc = rc.script('a256', 0)
    assert sc.actions.max() > 127  # bytes above int8


@pytest.mark.parametrize('name,seed', CASES)
def test_window_rule_is_the_stackers_encoded_observation(name, seed):
    from muzero_amd.replay import decode_state, encode_state

    sc = rc.script(name, seed)
    obs = rc.stacker_observations(name, seed)
    want = encode_state(obs, 'frames_u8', sc.frame_spec)
    got = rc.window_rows(sc)
    assert got.dtype == np.uint8 and got.shape == want.shape
    for m in range(rc.MOVES):
        assert got[m].tobytes() == want[m].tobytes(), (name, seed, m)
    back = decode_state(got, 'frames_u8', sc.frame_spec)
    assert back.dtype == np.float32 and (bits(back) == bits(obs)).all()


@pytest.mark.parametrize('rule', ['no_first', 'action_shift', 'plane_order'])
def test_the_data_tells_the_wrong_rules_apart(rule):
    for name, (C, *_rest) in rc.GEOMETRIES.items():
        if rule == 'plane_order' and C == 1:
            for seed in rc.SEEDS:  # (one channel: the two plane orders are the same order)
                sc = rc.script(name, seed)
                assert rc.window_rows(sc, rule).tobytes() == rc.window_rows(sc).tobytes()
            continue
        for seed in rc.SEEDS:
            sc = rc.script(name, seed)
            wrong, right = rc.window_rows(sc, rule), rc.window_rows(sc)
            assert (wrong != right).any(axis=1).sum() >= 5, (rule, name, seed)


def test_header_struct_is_the_ctypes_struct_with_record_format_last():
    from muzero_amd import planner

    text = open(os.path.join(REPO, 'include', 'mzplanner.h')).read()
    end = text.index('} mz_external_env;')
    body = text[text.rindex('typedef struct {', 0, end) + len('typedef struct {'):end]
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = re.findall(r'int32_t\s+([^;]+);', body)
    names = [n.strip() for f in fields for n in f.split(',')]
    assert names == [f for f, _ in planner.MzExternalEnv._fields_] and names[-1] == 'record_format'
    assert all(t is planner.C.c_int32 for _, t in planner.MzExternalEnv._fields_)
    assert re.search(r'#define MZ_RECORD_F32 0\b', text) and re.search(r'#define MZ_RECORD_FRAMES_U8 1\b', text)
    assert planner.RECORD_FORMATS == {'f32': 0, 'frames_u8': 1}
    assert 'mz_selfplay_record_info' in planner.ABI_SYMBOLS and re.search(r'\bint mz_selfplay_record_info\(', text)
    assert planner.MzExternalEnv().record_format == 0  # a zero-initialised struct asks for float32 records


def test_format_helper_refuses_unknown_names():
    from muzero_amd import pipeline, planner

    assert planner._record_format('f32') == 0 and planner._record_format('frames_u8') == 1
    for bad in ('u8', 'int8', '', None, 1, 0, True, b'f32'):
        with pytest.raises(ValueError, match='record_format'):
            planner._record_format(bad)
    import inspect

    for fn in (pipeline.run_self_play, planner.Planner.selfplay_reset_external):
        assert inspect.signature(fn).parameters['record_format'].default == 'f32'
