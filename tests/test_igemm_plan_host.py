"""Host only: the launch plans of the implicit-GEMM convolutions are the ones recorded before the kernels moved onto their shared
frame (csrc/igemm_tile.h; one K-cut-tail rule for plan_tiles and plan_b3 in csrc/conv_igemm.hip).

tests/golden/igemm_plans.json holds what tools/record_igemm_plans.py read from the library of the commit before that change:
mydet_conv_igemm_plan for every conv shape of tests/golden/conv_routes.json under the rule's own choice and each tile configuration
forced, mydet_conv_b3_plan plain and gated for the rows that hold the split-bf16 form, on 256 and on 64 CUs, with the workspace of
ops.WORKSPACE_BYTES and without one, and the shapes of tests/test_b3_plan_host.py under the MYDET_B3_* switches.  Every plan and
every return code must come out exactly as recorded.  Neither hook makes a GPU call."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'igemm_plans.json')


def _tool():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import record_igemm_plans
    finally:
        sys.path.pop(0)
    return record_igemm_plans


@pytest.fixture(scope='module')
def recorded():
    with open(GOLDEN) as f:
        return _tool().expand(json.load(f))


@pytest.fixture(scope='module')
def replayed(recorded):
    from mydetection_amd import _lib
    record_igemm_plans = _tool()
    saved = {k: os.environ.get(k) for k in record_igemm_plans.SWITCHES}
    try:
        return record_igemm_plans.replay(_lib.lib(), recorded)
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        _lib.lib().mydet_conv_b3_reload_tuning()


def test_the_recording_covers_what_it_should(recorded):
    from mydetection_amd import ops
    rec = _tool()
    shapes, b3 = rec.route_shapes()
    assert recorded['shapes'] == shapes and recorded['b3_shapes'] == b3 and len(shapes) > 100 and len(b3) > 50
    assert recorded['cfgs'] == [-1, 0, 1, 2, 3, 6, 8, 9] and recorded['cus'] == [256, 64] and recorded['ws'] == [ops.WORKSPACE_BYTES, 0]
    assert ['1', None, None] in recorded['settings'] and [None, '8', None] in recorded['settings']
    assert recorded['tuned_shapes'] == rec.tuned_shapes()
    n = len(recorded['cus']) * len(recorded['ws'])
    assert len(recorded['igemm']) == len(shapes) * len(recorded['cfgs']) * n
    assert len(recorded['b3']) == sum(2 if s[5] == 1 else 1 for s in b3) * n
    assert len(recorded['tuned']) == len(recorded['settings']) * len(recorded['tuned_shapes']) * n
    # a result is [code, out[0..6]]: out[4] workgroups of the main launch, out[5] tail tiles, out[6] cuts.  The recording reaches
    # both kinds of tail and an uncut grid in each family, a refusal, and all three split-bf16 forms
    for key in ('igemm', 'b3', 'tuned'):
        got = recorded[key]
        assert any(r[0] == 0 and r[5] > 0 and r[6] > 0 for r in got), key         # whole rounds + tail
        assert any(r[0] == 0 and r[5] == 0 and r[6] > 0 for r in got), key        # the whole grid cut
        assert any(r[0] == 0 and r[6] == 0 and r[7] == 1 for r in got), key       # uncut
    assert any(r[0] == -2 for r in recorded['tuned'])
    assert {r[1] for r in recorded['tuned'] if r[0] == 0} == {0, 1, 2}


@pytest.mark.parametrize('key', ['igemm', 'b3', 'tuned'])
def test_every_recorded_plan_is_reproduced(recorded, replayed, key):
    want, got = recorded[key], replayed[key]
    assert len(got) == len(want)
    wrong = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not wrong, f'{len(wrong)} of {len(want)} plans differ; first (index, recorded, now): {wrong[:3]}'
