"""GPU: every launch branch of the two Winograd kernels (csrc/conv_wino.hip F(2x2,3x3), csrc/conv_wino4.hip F(4x4,3x3)) against float64.

The counterpart of tests/test_gpu_igemm_tiles.py for the 3x3 stride-1 kernels.  No branch is guessed: every case first asks the launcher's
own arithmetic -- mydet_wino_plan with the device's CU count and ops.WORKSPACE_BYTES for F(2x2), mydet_wino4_tail_plan with 2 workgroups per
CU for F(4x4), `rn_log2` / `nbn` recomputed from Cout as w4_geometry does -- and asserts the plan the case was chosen for (the shapes are
for the 256 CUs of the MI355X; tests/test_host_cpu.py::test_wino_plan_rule pins the rule, ::test_wino_stream_k_partition the partition).

F(2x2), all NW = 8 (Cin >= 128), items = 64 tiles x 64 channels, nk = Cin / 8 slabs, `pieces` = partial tiles the fixup sums per item:
  a  plain 8-wave kernel, 129 .. 511 items: B = 1, 128 -> 1000, 47 x 45 (9 tile blocks x 16 = 144 items, the last block 40 of 64 tiles,
     ragged Cout) with (leaky, residual); the same at Cin = 136 (nk = 17: an odd slab count through the two-slab pipeline) with
     (swish, no residual) and (none, residual)
  b  a big grid whose tail is NOT covered (520 items: 8 tail items x 16 slabs < 256 workgroups) falls back to the plain kernel
  c  stream-K, whole rounds only: exactly 512 items, no tail, no fixup launch
  d  the smallest covered tail: 528 items, 16 tail items x 16 slabs = one slab per workgroup, every tail item 16 pieces
  e  small grid, nwg shrunk to the iteration count (2 items x 16 slabs on 32 workgroups): all six ACT x RES instances of
     conv_wino_fixup_kernel
  f  piece counts of the fixup's sums: 20 per item (Cin = 160 on 80 workgroups: the first piece + 16 + ONE partial trip of the
     eight-at-a-time loop) and 64 per item (B = 1, 512 -> 256, 4 items on all 256 workgroups: five whole trips + a partial one)
  g  a non-integral share: 24 items x 16 slabs on 256 workgroups, skq = 1, skr = 128 -- shares of 1 and 2 slabs alternate; by the host
     restatement (test_wino_stream_k_partition) every item is cut 11 ways and 8 workgroups own two slabs on either side of an item
     boundary: they leave slot 2w (the end of one item) AND slot 2w + 1 (the start of the next)
  h  the `small` boundary: exactly 128 items (half a round), 8 slabs per workgroup, every item cut in two
  n  (beyond the issue's list, found by the host walk) a tail of nearly a whole round, skq = nk - 1: four tail items are one
     workgroup's whole share, go through the MAIN kernel's epilogue, and their fixup workgroups take the "not cut" return
Every case: a second call is bit-identical; the workspace is pre-filled with a NaN bit pattern, and must still hold it everywhere after
a launch the plan says has no fixup, and be written by one that has; a launch with a fixup gives the same bits again over a zeroed
workspace (the fixup reads no slot that was not written).

F(4x4), `wino4=` only, so the pair of kernels runs whatever the item count; ids = 64-id blocks of RM x RN items, RN = 2^rn_log2:
  i  rn_log2 = 0 (Cout = 4, 32: blocks of 64 x 1) and 1 (Cout = 36, 64: 32 x 2) at B = 3, Cin = 88, 13 x 11 (ragged tiles, Cin % 32 != 0);
     Cout = 4 and 36 also at B = 9, 64 x 60: 68 tile blocks, so two / three block rows, the last one ragged
  j  a cut last column block with nbn = 2: Cout = 300 (ntn = 10: the second column block has 2 of 8 columns)
  k  the main kernel's (none, residual) and (swish, no residual) instances, on j's uncut shape
  l  the K-cut tail at its smallest: B = 17, 64 -> 512, 32 x 32 (544 items = one round of 512 + 32 items -- the ragged last block row,
     16 ids of each of its two blocks -- cut 4 ways), all six ACT x RES instances of wino4_fixup_kernel; each differs from the MYDET_W4_TAIL=0 launch and agrees with it within 2e-5 * max(1, max|plain|)
  m  a tail whose blocks include a cut column with nbn > 1: B = 17, 64 -> 292, 37 x 37 (ntn = 10, nbn = 2; 540 items; the tail is the
     last block row -- 6 tile blocks x (8 + 2) channel blocks, ids taken 48 per block, cut 4 ways -- so the second tail block has 12
     valid items among the 48 ids taken and the rest return in both the piece kernel and the fixup)

Bound: the project's own against a float64 reference of the same fused operation (tests/test_gpu_kernels.py: _conv_case), 2e-5 * max(1, max|ref|)
for F(2x2) and 6e-5 * ... for F(4x4).  The float64 conv runs on the CPU below 4 GFLOP and as the float64 ATen conv on the device above; it is
computed once per shape and shared by the epilogue variants."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from _arena import SENTINEL_BITS

pytestmark = pytest.mark.gpu

WS_BYTES = 64 << 20                 # ops.WORKSPACE_BYTES: what ops.conv2d hands the F(2x2) launcher
LEAKY_RES, LEAKY, SWISH_RES, SWISH, NONE_RES, NONE = (1, True), (1, False), (2, True), (2, False), (0, True), (0, False)
SIX = dict(leaky_res=LEAKY_RES, leaky=LEAKY, swish_res=SWISH_RES, swish=SWISH, none_res=NONE_RES, none=NONE)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from mydetection_amd import _lib
    _lib.lib()                                   # fail loudly if the HIP library is missing
    return torch.device('cuda:0')


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=2)
def _shape(B, Cin, Cout, H, W):
    """Seeded inputs of one shape (CPU, float32; as _conv_case draws them) and the float64 3x3 pad-1 conv of them, computed once: on
    the CPU below 4 GFLOP, as the float64 ATen conv on the device above.  Shared, and left unchanged, by the epilogue variants."""
    g = torch.Generator().manual_seed(1000 * Cin + Cout + 7 * H + W)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(B, Cout, H, W, generator=g)
    where = torch.device('cuda:0') if 2.0 * B * H * W * w.numel() > 4e9 else torch.device('cpu')
    conv = F.conv2d(x.to(where).double(), w.to(where).double(), None, 1, 1).cpu()
    return dict(x=x, w=w, scale=scale, shift=shift, res=res, conv=conv)


def _reference(s, act, residual):
    ref = s['conv'] * s['scale'].double().view(1, -1, 1, 1) + s['shift'].double().view(1, -1, 1, 1)
    if act == 1:
        ref = F.leaky_relu(ref, 0.1)
    elif act == 2:
        ref = ref * torch.sigmoid(ref)
    return ref + s['res'].double() if residual else ref


def _device_args(s, dev, residual):
    return dict(x=s['x'].to(dev).contiguous(memory_format=torch.channels_last), w=s['w'].permute(0, 2, 3, 1).contiguous().to(dev),
                scale=s['scale'].to(dev), shift=s['shift'].to(dev),
                res=s['res'].to(dev).contiguous(memory_format=torch.channels_last) if residual else None)


def _held(name, y, ref, rel):
    """|y - ref| against rel * max(1, max|ref|); prints the figure first."""
    assert tuple(y.shape) == tuple(ref.shape)
    yc = y.cpu().double()
    assert bool(torch.isfinite(yc).all()), f'{name}: non-finite output'
    tol = rel * max(1.0, ref.abs().max().item())
    err = (yc - ref).abs().max().item()
    print(f'wino_branches {name}: err {err:.3e} = {err / tol:.3f} of the bound {tol:.3e}')
    assert err <= tol, f'{name}: {err} > {tol}'


# ------------------------------------------------------------------------------------------------------------------------ F(2x2,3x3)
PLAIN = dict(nw=8, sk=0, nwg=0, tail=0, fixup=0)
F2_CASES = {
    'a_plain_leaky_res': dict(B=1, Cin=128, Cout=1000, H=47, W=45, ep=LEAKY_RES, plan=dict(PLAIN, items=144, nk=16)),
    'a_plain_nk17_swish': dict(B=1, Cin=136, Cout=1000, H=47, W=45, ep=SWISH, plan=dict(PLAIN, items=144, nk=17)),
    'a_plain_nk17_none_res': dict(B=1, Cin=136, Cout=1000, H=47, W=45, ep=NONE_RES, plan=dict(PLAIN, items=144, nk=17)),
    'b_not_covered_plain': dict(B=1, Cin=128, Cout=512, H=129, W=127, ep=LEAKY_RES, plan=dict(PLAIN, items=520, nk=16)),
    'c_whole_rounds': dict(B=2, Cin=128, Cout=1024, H=63, W=63, ep=LEAKY_RES,
                           plan=dict(nw=8, sk=1, items=512, nk=16, nwg=256, rounds=2, tail=0, skq=0, skr=0, fixup=0)),
    'd_smallest_tail': dict(B=1, Cin=128, Cout=1024, H=91, W=89, ep=SWISH_RES, pieces=16,
                            plan=dict(nw=8, sk=1, items=528, nk=16, nwg=256, rounds=2, tail=16, skq=1, skr=0, fixup=1)),
    **{f'e_small_{n}': dict(B=1, Cin=128, Cout=128, H=7, W=5, ep=ep, pieces=16,
                            plan=dict(nw=8, sk=1, items=2, nk=16, nwg=32, rounds=0, tail=2, skq=1, skr=0, fixup=1)) for n, ep in SIX.items()},
    'f_20_pieces': dict(B=1, Cin=160, Cout=256, H=15, W=13, ep=LEAKY, pieces=20,
                        plan=dict(nw=8, sk=1, items=4, nk=20, nwg=80, rounds=0, tail=4, skq=1, skr=0, fixup=1)),
    'f_64_pieces': dict(B=1, Cin=512, Cout=256, H=7, W=5, ep=LEAKY_RES, pieces=64,
                        plan=dict(nw=8, sk=1, items=4, nk=64, nwg=256, rounds=0, tail=4, skq=1, skr=0, fixup=1)),
    'g_non_integral_share': dict(B=1, Cin=128, Cout=384, H=31, W=29, ep=SWISH_RES,
                                 plan=dict(nw=8, sk=1, items=24, nk=16, nwg=256, rounds=0, tail=24, skq=1, skr=128, fixup=1)),
    'h_small_boundary': dict(B=2, Cin=128, Cout=256, H=63, W=63, ep=NONE, pieces=2,
                             plan=dict(nw=8, sk=1, items=128, nk=16, nwg=256, rounds=0, tail=128, skq=8, skr=0, fixup=1)),
    'n_uncut_tail_items': dict(B=7, Cin=128, Cout=768, H=47, W=47, ep=LEAKY_RES,
                               plan=dict(nw=8, sk=1, items=756, nk=16, nwg=256, rounds=2, tail=244, skq=15, skr=64, fixup=1)),
}


def _wino_plan(c):
    from mydetection_amd import _lib, ops
    assert ops.WORKSPACE_BYTES == WS_BYTES
    out = (ctypes.c_int32 * 10)()
    _lib.check(_lib.lib().mydet_wino_plan(c['B'], c['H'], c['W'], c['Cin'], c['Cout'], WS_BYTES, _cus(), out), 'mydet_wino_plan')
    return dict(zip(('nw', 'sk', 'items', 'nk', 'nwg', 'rounds', 'tail', 'skq', 'skr', 'fixup'), out))


@pytest.mark.parametrize('name', list(F2_CASES))
def test_wino_branch_vs_fp64(dev, name):
    from mydetection_amd import ops
    c = F2_CASES[name]
    plan = _wino_plan(c)
    assert {k: plan[k] for k in c['plan']} == c['plan'], (name, plan)
    if 'pieces' in c:               # equal shares that divide the items: every item is nk / skq pieces
        assert plan['skr'] == 0 and plan['nk'] % plan['skq'] == 0 and plan['nk'] // plan['skq'] == c['pieces'], (name, plan)
    act, residual = c['ep']
    s = _shape(c['B'], c['Cin'], c['Cout'], c['H'], c['W'])
    d = _device_args(s, dev, residual)
    u = ops.wino_weights(d['w'])
    assert u is not None and ops.WINOGRAD
    ws = ops.conv_workspace(dev)
    assert ws.numel() * 4 == WS_BYTES

    def run(bits):
        ws.view(torch.int32).fill_(bits)
        y = ops.conv2d(d['x'], d['w'], d['scale'], d['shift'], 3, 1, (1, 1, 1, 1), act, residual=d['res'], wino=u)
        torch.cuda.synchronize()
        return y

    y = run(SENTINEL_BITS)
    written = bool((ws.view(torch.int32) != SENTINEL_BITS).any())
    assert written == bool(plan['fixup']), f"{name}: workspace written = {written}, the plan's fixup = {plan['fixup']}"
    y2 = ops.conv2d(d['x'], d['w'], d['scale'], d['shift'], 3, 1, (1, 1, 1, 1), act, residual=d['res'], wino=u)
    assert torch.equal(y, y2), f'{name}: a second call differs'
    if plan['fixup']:
        y0 = run(0)
        assert torch.equal(y, y0), f'{name}: {int((y != y0).sum())} output value(s) depend on stale workspace contents'
    _held(name, y, _reference(s, act, residual), 2e-5)


# ------------------------------------------------------------------------------------------------------------------------ F(4x4,3x3)
SMALL4 = dict(B=3, Cin=88, H=13, W=11)
TAIL4 = dict(B=17, Cin=64, Cout=512, H=32, W=32)
F4_CASES = {
    'i_rn0_cout4': dict(SMALL4, Cout=4, ep=NONE, geo=(0, 1), ids=64, tail=()),
    'i_rn0_cout32': dict(SMALL4, Cout=32, ep=LEAKY_RES, geo=(0, 1), ids=64, tail=()),
    'i_rn1_cout36': dict(SMALL4, Cout=36, ep=SWISH_RES, geo=(1, 1), ids=64, tail=()),
    'i_rn1_cout64': dict(SMALL4, Cout=64, ep=LEAKY, geo=(1, 1), ids=64, tail=()),
    'i_rn0_two_block_rows': dict(B=9, Cin=88, Cout=4, H=64, W=60, ep=LEAKY_RES, geo=(0, 1), ids=128, tail=()),
    'i_rn1_three_block_rows': dict(B=9, Cin=88, Cout=36, H=64, W=60, ep=NONE, geo=(1, 1), ids=192, tail=()),
    'j_cut_column_nbn2': dict(SMALL4, Cout=300, ep=LEAKY_RES, geo=(3, 2), ids=128, tail=()),
    'k_none_res': dict(SMALL4, Cout=300, ep=NONE_RES, geo=(3, 2), ids=128, tail=()),
    'k_swish': dict(SMALL4, Cout=300, ep=SWISH, geo=(3, 2), ids=128, tail=()),
    # tail: (first id, blocks, ids per block, cuts) of the one group
    **{f'l_tail_{n}': dict(TAIL4, ep=ep, geo=(3, 2), ids=512, tail=(512, 2, 16, 4)) for n, ep in SIX.items()},
    'm_tail_cut_column': dict(B=17, Cin=64, Cout=292, H=37, W=37, ep=SWISH_RES, geo=(3, 2), ids=768, tail=(768, 2, 48, 4)),
}


def _w4_geometry(Cout):
    """(rn_log2, nbn) as w4_geometry of conv_wino4.hip derives them from the 32-channel block count."""
    ntn = (Cout + 31) // 32
    rn = 0
    while (1 << rn) < ntn and rn < 3:
        rn += 1
    return rn, (ntn + (1 << rn) - 1) >> rn


@pytest.mark.parametrize('name', list(F4_CASES))
def test_wino4_branch_vs_fp64(dev, name, monkeypatch):
    from mydetection_amd import _lib, ops
    c = F4_CASES[name]
    assert _w4_geometry(c['Cout']) == c['geo'], (name, _w4_geometry(c['Cout']))
    out = (ctypes.c_int32 * 17)()
    groups = _lib.lib().mydet_wino4_tail_plan(c['B'], c['H'], c['W'], c['Cin'], c['Cout'], 2 * _cus(), out)
    assert groups == (1 if c['tail'] else 0) and out[0] == c['ids'] and tuple(out[2:6]) == (c['tail'] or (0, 0, 0, 0)), (name, groups, list(out))
    act, residual = c['ep']
    s = _shape(c['B'], c['Cin'], c['Cout'], c['H'], c['W'])
    d = _device_args(s, dev, residual)
    u4 = ops.wino4_weights(d['w'])
    assert u4 is not None and ops.WINOGRAD and ops.WINOGRAD4

    def run():
        y = ops.conv2d(d['x'], d['w'], d['scale'], d['shift'], 3, 1, (1, 1, 1, 1), act, residual=d['res'], wino4=u4)
        torch.cuda.synchronize()
        return y

    y = run()
    assert torch.equal(y, run()), f'{name}: a second call differs'
    _held(name, y, _reference(s, act, residual), 6e-5)
    if c['tail']:                   # the tail did run: the uncut launch sums in another association
        monkeypatch.setenv('MYDET_W4_TAIL', '0')
        _lib.lib().mydet_wino4_reload_tuning()              # (the knobs are read once per process otherwise)
        try:
            plain = run()
        finally:
            monkeypatch.delenv('MYDET_W4_TAIL')
            _lib.lib().mydet_wino4_reload_tuning()
        assert not torch.equal(y, plain), f'{name}: the tail rule did not trigger on a shape chosen to trigger it'
        diff = (y - plain).abs().max().item()
        assert diff <= 2e-5 * max(1.0, plain.abs().max().item()), f'{name}: differs from the uncut launch by {diff}'
