"""Host only: the launch plan of the split-bf16 implicit GEMM (mydet_conv_b3_plan, csrc/conv_igemm.hip: plan_b3 -- the function
mydet_conv2d_igemm_b3_f32 takes its tile form, grid and K-cut tail from), pinned on a chip of 256 CUs on hand-worked shapes.

The rule, restated once.  Form: Cout <= 64 -> 128 x 64 tiles; otherwise, with T128 = ceil(M / 128) * ceil(Cout / 128), T128 <= HALF
(MYDET_B3_HALF_TILES, default cus / 2) -> 64 x 128 tiles; otherwise 128 x 128, or -- never with a gate -- 128 x 256 on 8 waves
(MYDET_B3_WIDE=1 and Cout > 192: form 1) or 128 x 128 on 8 waves (MYDET_B3_WAVES=8: form 2).  Grid: slots = 2 * cus (wide: cus),
total = tiles, rounds = total / slots, rem = total % slots, nk = ceil(K / 16), cuts = min(slots / rem, 16, nk / 8).  The remainder is cut
along K when cuts >= 2, the workspace holds rem * cuts * BM * BN floats, and either `small` (rounds == 0, total * 4 <= slots,
nk >= 32) or `rounds 2..4` (nk >= 64, 2 <= rounds <= 4, rem * 2 <= slots) holds.  (Either rule implies cuts >= 2 -- small: slots / rem
>= 4 and nk / 8 >= 4; rounds: slots / rem >= 2 and nk / 8 >= 8 -- so no shape shows `cuts >= 2` deciding on its own; the grid of
test_invariants_over_a_grid asserts it on every tail.)

Every shape is given as M rows (B = 1, Ho = 1, Wo = M): the factorisation of M does not enter the plan (asserted below)."""
import contextlib
import ctypes

import pytest

WS = 64 << 20                       # ops.WORKSPACE_BYTES
SWITCHES = ('MYDET_B3_WIDE', 'MYDET_B3_WAVES', 'MYDET_B3_HALF_TILES')
HUGE = str(1 << 30)


def _plan(M, Cin, Cout, taps=1, gated=0, ws=WS, cus=256):
    """mydet_conv_b3_plan as a dict, or the negative MYDET_E_* code."""
    from mydetection_amd import _lib
    out = (ctypes.c_int32 * 7)()
    rc = _lib.lib().mydet_conv_b3_plan(1, 1, M, Cin, Cout, taps, gated, ws, cus, out)
    if rc:
        return rc
    return dict(zip(('form', 'BM', 'BN', 'WN', 'main', 'tail', 'cuts'), out))


@contextlib.contextmanager
def _tuning(monkeypatch, wide=None, waves=None, half=None):
    """The three switches as given (None: unset), re-read by the library; unset and re-read again on the way out."""
    from mydetection_amd import _lib
    for name, value in zip(SWITCHES, (wide, waves, half)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    try:
        assert _lib.lib().mydet_conv_b3_reload_tuning() == (1 if str(wide) == '1' else 0) | (2 if str(waves) == '8' else 0)
        yield
    finally:
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        assert _lib.lib().mydet_conv_b3_reload_tuning() == 0


def _tile(p):
    return (p['form'], p['BM'], p['BN'], p['WN'])


UNCUT = dict(tail=0, cuts=1)
T64, T_HALF, T128, T_WAVES8, T_WIDE = (0, 128, 64, 2), (0, 64, 128, 2), (0, 128, 128, 2), (2, 128, 128, 4), (1, 128, 256, 4)


def test_form_boundaries(monkeypatch):
    with _tuning(monkeypatch):                                   # ---- default switches: HALF = cus / 2 = 128
        assert _tile(_plan(4096, 64, 64)) == T64 and _tile(_plan(1 << 18, 64, 64)) == T64 and _tile(_plan(64, 64, 1)) == T64
        # 65 channels: T128 decides.  128 row tiles x 1 channel tile = 128 -> 64-row tiles; one row more -> 129
        assert _tile(_plan(128 * 128, 64, 65)) == T_HALF and _tile(_plan(128 * 128 + 1, 64, 65)) == T128
        assert _tile(_plan(128 * 128, 64, 128)) == T_HALF and _tile(_plan(128 * 128 + 1, 64, 128)) == T128
        # two channel tiles: 64 x 2 = 128 / 65 x 2 = 130;  three: 42 x 3 = 126 / 43 x 3 = 129
        assert _tile(_plan(64 * 128, 64, 256)) == T_HALF and _tile(_plan(64 * 128 + 1, 64, 256)) == T128
        assert _tile(_plan(42 * 128, 64, 257)) == T_HALF and _tile(_plan(42 * 128 + 1, 64, 257)) == T128
        # the limit follows the chip: 304 CUs -> 152
        assert _tile(_plan(152 * 128, 64, 128, cus=304)) == T_HALF and _tile(_plan(152 * 128 + 1, 64, 128, cus=304)) == T128
        assert _tile(_plan(1 << 18, 64, 1024)) == T128           # no opt-in form without its switch
    with _tuning(monkeypatch, half=0):                           # ---- never 64-row tiles
        assert _tile(_plan(1, 64, 65)) == T128 and _tile(_plan(128, 64, 128)) == T128 and _tile(_plan(1, 64, 64)) == T64
    with _tuning(monkeypatch, half=HUGE):                        # ---- always, above 64 channels
        assert _tile(_plan(1 << 18, 64, 1024)) == T_HALF and _tile(_plan(1 << 18, 64, 65)) == T_HALF
        assert _tile(_plan(1 << 18, 64, 64)) == T64
    with _tuning(monkeypatch, half=129):                         # (the value is the limit itself)
        assert _tile(_plan(129 * 128, 64, 128)) == T_HALF and _tile(_plan(129 * 128 + 1, 64, 128)) == T128
    with _tuning(monkeypatch, wide=1, half=0):                   # ---- wide: only past 192 channels
        assert _tile(_plan(4096, 64, 192)) == T128 and _tile(_plan(4096, 64, 193)) == T_WIDE and _tile(_plan(4096, 64, 64)) == T64
        assert _tile(_plan(4096, 64, 256, gated=1)) == T128      # no gated instance: the default form
    with _tuning(monkeypatch, waves=8, half=0):                  # ---- 8 waves: every 128 x 128 launch, not the 128 x 64 one
        assert _tile(_plan(4096, 64, 65)) == T_WAVES8 and _tile(_plan(4096, 64, 1024)) == T_WAVES8 and _tile(_plan(4096, 64, 64)) == T64
        assert _tile(_plan(4096, 64, 128, gated=1)) == T128
    with _tuning(monkeypatch, wide=1, waves=8, half=0):          # both: wide wins past 192 channels
        assert _tile(_plan(4096, 64, 192)) == T_WAVES8 and _tile(_plan(4096, 64, 193)) == T_WIDE
    with _tuning(monkeypatch, wide=1, waves=8):                  # the 64-row rule comes before either opt-in form
        assert _tile(_plan(64 * 128, 64, 256)) == T_HALF and _tile(_plan(64 * 128 + 1, 64, 256)) == T_WIDE
        assert _tile(_plan(128 * 128, 64, 128)) == T_HALF and _tile(_plan(128 * 128 + 1, 64, 128)) == T_WAVES8
    with _tuning(monkeypatch, wide=0, waves=4):                  # other values of the switches: off
        assert _tile(_plan(1 << 18, 64, 1024)) == T128


def test_gated_project_convs_of_a_lane_of_eight(monkeypatch):
    """The MBConv project convs of EfficientDet-D1 on a lane of 8 images (20 x 20 maps: M = 3 200), default switches."""
    with _tuning(monkeypatch):
        # 1152 -> 192: T128 = 25 x 2 = 50 <= 128 -> 64-row tiles, 50 x 2 = 100 tiles; small (400 <= 512, nk = 72);
        # cuts = min(512 / 100, 16, 72 / 8) = min(5, 16, 9) = 5: all 100 tiles cut five ways, nothing in the main launch
        assert _plan(3200, 1152, 192, gated=1) == dict(form=0, BM=64, BN=128, WN=2, main=0, tail=100, cuts=5)
        # 672 -> 112: one channel tile, 50 tiles, small, nk = 42, cuts = min(10, 16, 5) = 5
        assert _plan(3200, 672, 112, gated=1) == dict(form=0, BM=64, BN=128, WN=2, main=0, tail=50, cuts=5)
        # the gate does not enter the grid
        assert _plan(3200, 1152, 192) == _plan(3200, 1152, 192, gated=1)
        # on a lane of 16 (M = 6 400): T128 = 100 -> 64-row tiles, 200 of them, 800 > 512: not small, no whole round: uncut
        assert _plan(6400, 1152, 192, gated=1) == dict(form=0, BM=64, BN=128, WN=2, main=200, **UNCUT)


def test_small_rule(monkeypatch):
    with _tuning(monkeypatch, half=0):                           # 128 x 128 tiles at any size, one channel tile: tiles = M / 128
        t = lambda tiles, Cin, **kw: _plan(tiles * 128, Cin, 128, **kw)        # noqa: E731
        # total * 4 <= slots: 128 tiles yes (cuts = min(4, 16, 32 / 8) = 4), 129 no
        assert t(128, 512) == dict(form=0, BM=128, BN=128, WN=2, main=0, tail=128, cuts=4)
        assert t(129, 512) == dict(form=0, BM=128, BN=128, WN=2, main=129, **UNCUT)
        # nk >= 32: Cin = 496 is 31 slabs, 500 is 32 (the last one short)
        assert t(128, 496)['tail'] == 0 and t(128, 500) == t(128, 512) and t(1, 496)['tail'] == 0
        # cuts = min(slots / rem, 16, nk / 8), each term in turn
        assert (t(100, 4096)['tail'], t(100, 4096)['cuts']) == (100, 5)        # 512 / 100
        assert (t(40, 4096)['tail'], t(40, 4096)['cuts']) == (40, 12)          # 512 / 40
        assert (t(20, 4096)['tail'], t(20, 4096)['cuts']) == (20, 16)          # the cap
        assert (t(1, 4096)['tail'], t(1, 4096)['cuts']) == (1, 16)
        assert (t(20, 640)['tail'], t(20, 640)['cuts']) == (20, 5)             # nk / 8 = 40 / 8
        assert t(20, 1008)['cuts'] == 7 and t(20, 1012)['cuts'] == 8           # 63 slabs: 63 / 8 = 7; 64 slabs, the last one short: 8
        # the 3x3 shape of the GPU module: 150 rows are 2 tiles, K = 9 x 64 is 36 slabs: cuts = 36 / 8 = 4
        assert _plan(150, 64, 136, taps=9) == dict(form=0, BM=128, BN=128, WN=2, main=0, tail=4, cuts=4)
    with _tuning(monkeypatch):
        # at the default HALF the 128 x 128 form needs T128 > 128 and `small` needs total <= 128: never both
        for tiles in (1, 64, 128, 129, 200, 511, 512, 513, 700):
            for Cout in (65, 128, 129, 256, 1024):
                p = _plan(tiles * 128, 4096, Cout)
                if (p['BM'], p['BN']) == (128, 128):
                    assert p['main'] > 0, (tiles, Cout, p)
        # the 64 x 128 and 128 x 64 forms do reach it
        assert _plan(150, 768, 136) == dict(form=0, BM=64, BN=128, WN=2, main=0, tail=6, cuts=6)
        assert _plan(150, 768, 48) == dict(form=0, BM=128, BN=64, WN=2, main=0, tail=2, cuts=6)


def test_rounds_rule(monkeypatch):
    with _tuning(monkeypatch, half=0):
        t = lambda tiles, Cin=1024, **kw: _plan(tiles * 128, Cin, 128, **kw)   # noqa: E731
        cut = lambda main, tail, cuts: dict(form=0, BM=128, BN=128, WN=2, main=main, tail=tail, cuts=cuts)     # noqa: E731
        # two rounds of 512 + 40 tiles, 64 slabs: cuts = min(512 / 40, 16, 64 / 8) = 8;  63 slabs: uncut
        assert t(1064) == cut(1024, 40, 8) and t(1064, 1008) == cut(1064, 0, 1) and t(1064, 1012) == cut(1024, 40, 8)
        # rounds 1, 2, 3, 4, 5
        assert t(552) == cut(552, 0, 1) and t(1576) == cut(1536, 40, 8) and t(2088) == cut(2048, 40, 8) and t(2600) == cut(2600, 0, 1)
        # whole rounds: nothing to cut
        assert t(1024) == cut(1024, 0, 1) and t(2048) == cut(2048, 0, 1)
        # rem * 2 <= slots: 256 tiles yes (two ways), 257 no
        assert t(1024 + 256) == cut(1024, 256, 2) and t(1024 + 257) == cut(1024 + 257, 0, 1)
        assert t(1024 + 1, 4096) == cut(1024, 1, 16) and t(1024 + 32, 4096) == cut(1024, 32, 16) and t(1024 + 33, 4096) == cut(1024, 33, 15)
        # between a quarter round and two rounds: neither rule
        for tiles in (129, 256, 511, 513, 1023):
            assert t(tiles, 4096) == cut(tiles, 0, 1), tiles
        # the workspace: 40 tiles x 8 slices x 128 x 128 floats; none, or a byte short: uncut
        need = 40 * 8 * 128 * 128 * 4
        assert t(1064, ws=need) == cut(1024, 40, 8)
        for short in (0, -1, need - 1):
            assert t(1064, ws=short) == cut(1064, 0, 1), short
        need = 128 * 4 * 128 * 128 * 4                           # ... and the small rule's
        assert t(128, 512, ws=need)['tail'] == 128 and t(128, 512, ws=need - 1)['tail'] == 0 and t(128, 512, ws=0)['tail'] == 0
        # another chip size moves the rounds: 304 CUs hold 608 tiles at once
        assert t(1064, cus=304) == cut(1064, 0, 1) and t(1216 + 40, cus=304) == cut(1216, 40, 8)
    with _tuning(monkeypatch):
        # default switches: the shape of the GPU module's case (1 064 tiles of 128 rows), and Darknet-53's 1024 -> 512 at 20 x 20
        assert _plan(1064 * 128, 1024, 128) == dict(form=0, BM=128, BN=128, WN=2, main=1024, tail=40, cuts=8)
        assert _plan(128 * 400, 1024, 512) == dict(form=0, BM=128, BN=128, WN=2, main=1536, tail=64, cuts=8)          # batch 128: 3 rounds + 64
        assert _plan(40 * 400, 1024, 512) == dict(form=0, BM=128, BN=128, WN=2, main=500, **UNCUT)                     # batch 40: under a round
        assert _plan(82 * 400, 1024, 512) == dict(form=0, BM=128, BN=128, WN=2, main=1024, tail=4, cuts=8)             # batch 82: the first with 2 rounds
        assert _plan(81 * 400, 1024, 512)['tail'] == 0 and _plan(112 * 400, 1024, 512)['tail'] == 0                   # (112: rem 376 > 256)


def test_wide_form(monkeypatch):
    with _tuning(monkeypatch, wide=1, half=0):
        t = lambda tiles, Cin=1152, **kw: _plan(tiles * 128, Cin, 256, **kw)   # noqa: E731
        cut = lambda main, tail, cuts: dict(form=1, BM=128, BN=256, WN=4, main=main, tail=tail, cuts=cuts)     # noqa: E731
        # slots = cus = 256: 552 tiles are two rounds + 40, nk = 1152 / 16 = 72: cuts = min(256 / 40, 16, 9) = 6 ...
        assert t(552) == cut(512, 40, 6)
        assert _plan(552 * 128, 128, 256, taps=9) == cut(512, 40, 6)           # (K = taps x Cin)
        # ... where the 4-wave form (512 slots) has one round and no tail
        assert _plan(552 * 128, 1152, 128) == dict(form=0, BM=128, BN=128, WN=2, main=552, **UNCUT)
        # rounds 1, 4, 5;  rem * 2 <= 256;  nk = 63 / 64
        assert t(296) == cut(296, 0, 1) and t(1064) == cut(1024, 40, 6) and t(1320) == cut(1320, 0, 1)
        assert t(512 + 128) == cut(512, 128, 2) and t(512 + 129) == cut(512 + 129, 0, 1)
        assert t(552, 1008) == cut(552, 0, 1) and t(552, 1024) == cut(512, 40, 6)
        # small: total * 4 <= 256
        assert t(64, 512) == cut(0, 64, 4) and t(65, 512) == cut(65, 0, 1) and t(64, 496) == cut(64, 0, 1) and t(16, 4096) == cut(0, 16, 16)
        # two channel tiles
        assert _plan(276 * 128, 1152, 257) == cut(512, 40, 6)
        # the workspace
        need = 40 * 6 * 128 * 256 * 4
        assert t(552, ws=need) == cut(512, 40, 6) and t(552, ws=need - 1) == cut(552, 0, 1) and t(552, ws=0) == cut(552, 0, 1)
        # cus is the round: 304
        assert t(552, cus=304) == cut(552, 0, 1) and t(608 + 40, cus=304) == cut(608, 40, 7)
        # no padded-K instance: Cin % 16 past 192 channels is refused, and only there, and only under this switch
        assert _plan(4096, 40, 260) == -2 and _plan(4096, 40, 193) == -2 and _tile(_plan(4096, 40, 192)) == T128
        assert _tile(_plan(4096, 48, 260)) == T_WIDE
    with _tuning(monkeypatch):
        assert _tile(_plan(4096, 40, 260)) == T_HALF


def test_eight_wave_form_uses_the_same_grid(monkeypatch):
    with _tuning(monkeypatch, waves=8, half=0):
        w8 = [_plan(tiles * 128, Cin, 128) for tiles in (1, 128, 129, 552, 1064, 1281, 2600) for Cin in (496, 512, 1008, 1024)]
    with _tuning(monkeypatch, half=0):
        w4 = [_plan(tiles * 128, Cin, 128) for tiles in (1, 128, 129, 552, 1064, 1281, 2600) for Cin in (496, 512, 1008, 1024)]
    assert [dict(p, form=0, WN=2) for p in w8] == w4 and all(_tile(p) == T_WAVES8 for p in w8)
    assert any(p['tail'] and p['main'] for p in w8) and any(p['tail'] and not p['main'] for p in w8)


def test_invariants_over_a_grid(monkeypatch):
    """Every plan of a grid of shapes, under each setting of the switches: tiles add up, a tail has 2..min(16, nk / 8) cuts that fit
    the workspace, and nothing is cut without one."""
    cins = (16, 32, 40, 64, 96, 256, 496, 512, 768, 1008, 1024, 1152, 4608)
    couts = (8, 48, 64, 65, 112, 128, 129, 192, 193, 255, 256, 264, 512, 1024)
    rows = (1, 150, 189, 3200, 6400, 16384, 16385, 51200, 70656, 136192, 1 << 18, 1 << 20)
    tails = {}
    for setting in (dict(), dict(half=0), dict(half=HUGE), dict(half=0, waves=8), dict(half=0, wide=1)):
        with _tuning(monkeypatch, **setting):
            for Cin in cins:
                for Cout in couts:
                    for taps in (1, 9):
                        for M in rows:
                            for ws in (WS, 1 << 20, 0):
                                p = _plan(M, Cin, Cout, taps, ws=ws)
                                if p == -2:             # channel counts no form takes, or an output past the 32-bit byte offsets
                                    assert ((Cin % 16 and taps == 9) or (Cin % 16 and setting.get('wide') and Cout > 192)
                                            or M * Cout * 4 >= 0x7FFFFFF0), (M, Cin, Cout, taps)
                                    continue
                                assert _tile(p) in (T64, T_HALF, T128, T_WAVES8, T_WIDE), p
                                assert (Cout <= 64) == (_tile(p) == T64) and (p['form'] == 1) <= (Cout > 192), (p, Cout)
                                total = -(-M // p['BM']) * -(-Cout // p['BN'])
                                nk = -(-(taps * Cin) // 16)
                                assert p['main'] + p['tail'] == total and p['main'] >= 0 and p['tail'] >= 0, (p, M, Cin, Cout, taps)
                                assert (p['cuts'] == 1) == (p['tail'] == 0), p
                                if p['tail']:
                                    assert 2 <= p['cuts'] <= min(16, nk // 8) and nk >= 32, (p, M, Cin, Cout, taps)
                                    assert p['tail'] * p['cuts'] * p['BM'] * p['BN'] * 4 <= ws, (p, M, Cin, Cout, taps)
                                    assert p['main'] % ((1 if p['form'] == 1 else 2) * 256) == 0, p
                                    key = (_tile(p), 'small' if p['main'] == 0 else 'rounds')
                                    tails[key] = tails.get(key, 0) + 1
    # both kinds of tail occur on every form (the `small` one of the 4-wave 128 x 128 form: only with HALF = 0, asserted in test_small_rule)
    assert set(tails) == {(t, k) for t in (T64, T_HALF, T128, T_WAVES8, T_WIDE) for k in ('small', 'rounds')}, sorted(tails)


def test_arguments(monkeypatch):
    from mydetection_amd import _lib
    fn = _lib.lib().mydet_conv_b3_plan
    out = (ctypes.c_int32 * 7)()
    with _tuning(monkeypatch):
        assert fn(11, 80, 80, 1024, 128, 1, 0, WS, 256, out) == 0 and list(out) == [0, 128, 128, 2, 550, 0, 1]     # 550 tiles: one round + 38
        assert dict(zip(('form', 'BM', 'BN', 'WN', 'main', 'tail', 'cuts'), out)) == _plan(70400, 1024, 128)     # M, not its factors
        for bad in ((0, 80, 80, 1024, 128, 1, 0, WS, 256), (11, 0, 80, 1024, 128, 1, 0, WS, 256), (11, 80, -1, 1024, 128, 1, 0, WS, 256),
                    (11, 80, 80, 0, 128, 1, 0, WS, 256), (11, 80, 80, 1024, 0, 1, 0, WS, 256), (11, 80, 80, 1024, 128, 0, 0, WS, 256),
                    (11, 80, 80, 1024, 128, 1, 0, WS, 0), (11, 80, 80, 1024, 128, 1, 0, WS, (1 << 20) + 1),
                    (11, 80, 80, 1024, 128, 9, 1, WS, 256),                    # a gate on a 3x3 layer
                    (1 << 11, 1 << 10, 1 << 10, 1024, 128, 1, 0, WS, 256)):    # more than 2^30 rows
            assert fn(*bad, out) == -1, bad
        assert fn(11, 80, 80, 1024, 128, 1, 0, WS, 256, None) == -1
        # channel counts: Cin % 16 only with one tap, and then Cin % 4
        assert _plan(4096, 24, 128, taps=9) == -2 and _plan(4096, 24, 128) != -2 and _plan(4096, 22, 128) == -2 and _plan(4096, 6, 128) == -2
        assert _plan(4096, 40, 128, gated=1) == dict(form=0, BM=64, BN=128, WN=2, main=64, **UNCUT)
        assert _plan(4096, 16, 128, taps=32) == -2               # more taps than the kernel's tap table
        # an output past 2 GiB - 16 bytes at ldy = Cout, as the entry point: 2^22 rows of 128 channels; 2^30 rows of 2^20
        assert _plan(1 << 22, 64, 128) == -2 and _plan((1 << 22) - 1, 64, 128)['main'] == 1 << 15 and _plan(1 << 30, 4, 1 << 20) == -2
    # mydet_conv_b3_reload_tuning: the form bits as before, and MYDET_B3_HALF_TILES is read again with them
    for half, want in ((None, T_HALF), (0, T128), (1, T128), (HUGE, T_HALF)):
        with _tuning(monkeypatch, half=half):
            assert _tile(_plan(256, 64, 128)) == want, half
    monkeypatch.setenv('MYDET_B3_HALF_TILES', '0')               # set but not re-read: the old value holds
    assert _tile(_plan(256, 64, 128)) == T_HALF
    monkeypatch.delenv('MYDET_B3_HALF_TILES')
    assert _lib.lib().mydet_conv_b3_reload_tuning() == 0


def test_ops_wrapper(monkeypatch):
    from mydetection_amd import ops
    with _tuning(monkeypatch):
        assert ops.b3_plan(8, 20, 20, 1152, 192, 1, gated=True) == ops.B3Plan(form=0, bm=64, bn=128, wn=2, main=0, tail=100, cuts=5)
        assert ops.b3_plan(8, 20, 20, 1152, 192, 1, workspace_bytes=0).tail == 0 and ops.b3_plan(1, 8, 8, 24, 128, 9) == -2
        assert ops.WORKSPACE_BYTES == WS


@pytest.mark.parametrize('case,want', [
    # the cases of tests/test_gpu_kernels.py: test_conv_split_bf16_vs_fp64 that its comments describe, as facts (M, Cin, Cout, taps)
    ((32 * 32 * 32, 32, 64, 9), dict(form=0, BM=128, BN=64, WN=2, main=256, **UNCUT)),
    ((16 * 1600, 256, 128, 1), dict(form=0, BM=128, BN=128, WN=2, main=200, **UNCUT)),
    ((40 * 400, 1024, 512, 1), dict(form=0, BM=128, BN=128, WN=2, main=500, **UNCUT)),
    ((16 * 400, 1152, 192, 1), dict(form=0, BM=64, BN=128, WN=2, main=200, **UNCUT)),          # gated: 200 tiles of 64 rows, not cut
    ((16 * 1600, 672, 112, 1), dict(form=0, BM=128, BN=128, WN=2, main=200, **UNCUT)),         # 200 tiles of 128 x 128: above the limit
    ((8 * 1600, 480, 80, 1), dict(form=0, BM=64, BN=128, WN=2, main=200, **UNCUT)),
    ((5 * 33 * 31, 96, 64, 1), dict(form=0, BM=128, BN=64, WN=2, main=40, **UNCUT)),           # nk = 6: too short to cut
    ((8 * 100, 192, 1152, 1), dict(form=0, BM=64, BN=128, WN=2, main=117, **UNCUT)),           # 63 tiles of 128 x 128 -> 13 x 9 of 64 x 128
    ((40 * 1600, 672, 112, 1), dict(form=0, BM=128, BN=128, WN=2, main=500, **UNCUT)),
])
def test_plans_of_the_existing_gpu_cases(monkeypatch, case, want):
    with _tuning(monkeypatch):
        assert _plan(*case) == want
