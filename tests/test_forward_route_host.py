"""What the forward pass's one route (csrc/fc_forward_route.hpp) decides, read from fc_describe_kernels and the size queries on any
machine: the schedule of every launch equals the restatement of the rules as they stood before the route existed
(tests/_forward_schedule_ref.py), and the packed forward image has the layout the launch will read."""
import ctypes
import os
import re

import pytest

import _forward_schedule_ref as ref
from fieldconv_amd import _env, _lib

SHAPES = [(16, 16, 4, 1), (64, 64, 6, 3)]                 # (I, O, R, B)
MODES = {'split': 0, 'f32': 1, 'f16': 2}                  # fc_dims::mode
KINDS = (0, 1, 2)
# every N up to 20 000 with sparse supports (no edge split), and three small meshes with 128 neighbours (the edge split)
MESHES = [(N, 8 * N) for N in range(1, 20001)] + [(N, 128 * N) for N in (48, 200, 1024)]
FIELDS = re.compile(r' grid=(\d+) whole=(\d+) half=(\d+) spread=([01]) lds=(\d+) cus=(\d+)(?: slabs=([12]))?;')


def _defaults_or_skip():
    on = [k for k in _env.LIBRARY_SWITCHES if os.environ.get(k) not in (None, '')]
    if on:
        pytest.skip('development switches set (%s): the restatement is of the default rules' % ', '.join(on))


def _describe(lib, buf, N, E, I, O, R, B, mode, kind):
    d = _lib.FcDims(N, E, I, O, R, B, mode=mode)
    assert lib.fc_describe_kernels(ctypes.byref(d), kind, buf, len(buf)) == 0, (N, E, I, O, R, B, mode, kind)
    text = buf.value.decode()
    m = FIELDS.search(text)
    assert m, text
    fwd = text[:m.end()]
    parts = re.search(r'parts=(\d+)\)', fwd)
    got = dict(arrangement='ring-major' if '(ring-major' in fwd else 'frequency-major', grid=int(m.group(1)), whole=int(m.group(2)),
               half=int(m.group(3)), spread=int(m.group(4)))
    if parts:                                              # (the ring-major text names no parts)
        got['parts'] = int(parts.group(1))
    assert ('(frequency-major' in fwd) != ('(ring-major' in fwd), fwd
    assert (m.group(7) is not None) == (got['arrangement'] == 'frequency-major'), fwd
    return got, int(m.group(6)), d


@pytest.mark.parametrize('mode', sorted(MODES))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'I%d-O%d-R%d-B%d' % s)
def test_schedule_and_image_equal_the_restatement_of_the_earlier_rules(shape, mode):
    _defaults_or_skip()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1536)
    I, O, R, B = shape
    cus = _describe(lib, buf, 100, 800, I, O, R, B, MODES[mode], 1)[1]
    if cus != 256:
        pytest.skip('the description says cus=%d: the expected figures are the MI355X\'s (256 CUs)' % cus)
    freq_floats, ring_floats = ref.frequency_image_floats(I, O, R, B, MODES[mode]), ref.ring_image_floats(I, O, R, B, MODES[mode])
    seen = set()
    for N, E in MESHES:
        for kind in KINDS:
            got, _, d = _describe(lib, buf, N, E, I, O, R, B, MODES[mode], kind)
            want = ref.schedule(N, E, kind, MODES[mode], 256)
            if 'parts' not in got:
                assert want['parts'] == 1, (N, E, kind, got, want)
                got['parts'] = 1
            assert got == want, (N, E, kind, got, want)
            if kind == 0:
                assert got['grid'] == (N + 15) // 16 and got['half'] == 0
            # pack and launch agree: the image has the ring layout's size exactly when the launch is ring-major
            floats = lib.fc_packed_filter_floats_fwd(ctypes.byref(d), 1 if kind else 0)
            assert floats == (ring_floats if got['arrangement'] == 'ring-major' else freq_floats), (N, E, kind, floats)
            seen.add((got['arrangement'], got['half'] > 0, got['spread'], got['parts'] > 1))
    if mode == 'split':        # every branch of the three rules was met
        assert {('ring-major', True, 1, False), ('ring-major', True, 0, False), ('ring-major', False, 0, False),
                ('frequency-major', False, 0, True), ('frequency-major', False, 0, False)} <= seen, seen
    else:
        assert ('frequency-major', True, 0, False) in seen and not any(s[0] == 'ring-major' for s in seen), seen


POINTS = [      # (N, E, kind, mode) -> the fields that must come out, on 256 CUs
    ((4112, 8 * 4112, 1, 'split'), dict(arrangement='ring-major', grid=512, whole=2, half=510, spread=1)),
    ((8203, 8 * 8203, 1, 'split'), dict(arrangement='ring-major', grid=512, whole=512, half=2, spread=0)),
    ((12300, 8 * 12300, 1, 'split'), dict(arrangement='ring-major', grid=512, whole=769, half=0)),
    ((4112, 8 * 4112, 1, 'f32'), dict(arrangement='frequency-major', grid=256, whole=256, half=2)),
    ((3000, 8 * 3000, 1, 'split'), dict(arrangement='frequency-major', grid=188, half=0)),
    ((1024, 131072, 1, 'split'), dict(arrangement='frequency-major', parts=4, grid=256)),
    ((1024, 131072, 0, 'split'), dict(arrangement='frequency-major', grid=64, whole=64, half=0)),
]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'I%d-O%d-R%d-B%d' % s)
@pytest.mark.parametrize('point,want', POINTS, ids=lambda p: '-'.join(map(str, p)) if isinstance(p, tuple) else None)
def test_named_points_of_the_schedule(point, want, shape):
    _defaults_or_skip()
    lib = _lib.load()
    buf = ctypes.create_string_buffer(1536)
    N, E, kind, mode = point
    got, cus, _ = _describe(lib, buf, N, E, *shape, MODES[mode], kind)
    if cus != 256:
        pytest.skip('the description says cus=%d: the expected figures are the MI355X\'s (256 CUs)' % cus)
    assert {k: got.get(k) for k in want} == want, (got, buf.value)
