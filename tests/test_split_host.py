"""The conv_precision switch on the host side (no GPU): make_mz_config's parsing, the header's field and constants, and the ctypes
mirror's size against the field list of the header."""
import ctypes as C
import os
import re

import pytest

from helpers import REPO, build_conv, conv_case

HEADER = os.path.join(REPO, 'include', 'mzplanner.h')


def _spec():
    return build_conv(conv_case('board3')).planner_spec()


def test_make_mz_config_reads_conv_precision():
    from muzero_amd import planner as pl

    spec = _spec()
    assert pl.make_mz_config(spec, None).conv_precision == 0
    assert pl.make_mz_config(spec, None, conv_precision='bf16x3').conv_precision == 1
    assert pl.make_mz_config(spec, None, conv_precision='f32').conv_precision == 0
    assert pl.make_mz_config(spec, None, conv_precision=1).conv_precision == 1
    assert pl.make_mz_config(spec, None, conv_precision=0).conv_precision == 0

    class Cfg:
        conv_precision = 'bf16x3'

    assert pl.make_mz_config(spec, Cfg()).conv_precision == 1
    assert pl.make_mz_config(spec, Cfg(), conv_precision='f32').conv_precision == 0  # the keyword wins, like the other overrides


@pytest.mark.parametrize('bad', ['bf16', 'fp32', 2, -1, None, 1.5, True])
def test_unknown_conv_precision_raises(bad):
    from muzero_amd import planner as pl

    with pytest.raises(ValueError, match='conv_precision'):
        pl.make_mz_config(_spec(), None, conv_precision=bad)


def _header_config_fields():
    """(ctype, name) of every field of mz_config, from the header text (comments stripped), in order."""
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    body = re.search(r'typedef\s+struct\s*\{([^}]*)\}\s*mz_config\s*;', text).group(1)
    ctypes_of = {'int32_t': C.c_int32, 'uint64_t': C.c_uint64, 'double': C.c_double}
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        fields += [(ctypes_of[typ], n.strip()) for n in names.split(',')]
    return fields


def test_header_declares_field_and_constants():
    text = open(HEADER).read()
    assert re.search(r'^#define\s+MZ_CONV_F32\s+0\b', text, flags=re.M)
    assert re.search(r'^#define\s+MZ_CONV_BF16X3\s+1\b', text, flags=re.M)
    fields = _header_config_fields()
    assert fields[-1] == (C.c_int32, 'conv_precision')  # trailing, after legacy_scalar_promotion
    assert fields[-2] == (C.c_int32, 'legacy_scalar_promotion')


def test_ctypes_mirror_matches_the_header():
    from muzero_amd import planner as pl

    fields = _header_config_fields()
    assert [(n, t) for t, n in fields] == list(pl.MzConfig._fields_)

    class FromHeader(C.Structure):
        _fields_ = [(n, t) for t, n in fields]

    assert C.sizeof(pl.MzConfig) == C.sizeof(FromHeader)
    assert pl.MzConfig.conv_precision.offset == FromHeader.conv_precision.offset
