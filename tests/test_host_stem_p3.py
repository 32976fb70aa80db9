"""CPU-only checks of the fused stem + stride-2 conv launch (csrc/conv_stem_p3.hip): tile plan and LDS bytes of the bench shapes, the
dispatch rule, the exported symbol, and -- read from the built library's code-object metadata -- the registers, scratch and LDS that
the source comment's occupancy claim (two workgroups of four waves per CU, as conv_p3_kernel) needs."""
import ctypes
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024             # MI355X
VGPRS_PER_SIMD_LANE = 512           # unified vector + accumulation registers; two waves per SIMD leave 256 each


def test_tile_plan_and_lds_bytes():
    from mydetection_amd import _lib, ops
    lds = 3 * 17 * 36 * 32 + 3 * 19 * 36 * 4
    assert lds == 66960 and _lib.lib().mydet_conv_stem_p3_lds_bytes() == lds
    assert 2 * lds <= LDS_PER_CU < 3 * lds                          # two workgroups per CU, by LDS
    assert lds + 3 * 17 * 36 * 32 > LDS_PER_CU // 2                 # ... which a second resident slab would not leave
    assert ops.stem_p3_plan(32, 640, 640, 64) == (32 * 40 * 20, lds)
    assert ops.stem_p3_plan(32, 512, 512, 64) == (32 * 32 * 16, lds)
    assert ops.stem_p3_plan(1, 512, 512, 64) == (32 * 16, lds)
    assert ops.stem_p3_plan(2, 40, 72, 128) == (2 * 3 * 3 * 2, lds)  # ragged tiles in both directions, two channel tiles
    assert ops.stem_p3_plan(1, 37, 51, 64) == (3 * 2, lds)


def test_dispatch_rule(monkeypatch):
    from mydetection_amd import ops
    pad = (1, 1, 1, 1)
    monkeypatch.setattr(ops, 'STEM_P3', True)
    for B, H, W in ((32, 640, 640), (32, 512, 512), (1, 512, 512)):
        assert ops.stem_p3_takes(B, H, W, 64, pad) == ops.p3_takes(B, H // 2, W // 2, 32, 64, 3, 2, pad), (B, H, W)
    assert ops.stem_p3_takes(32, 640, 640, 64, pad)
    assert not ops.stem_p3_takes(32, 640, 640, 96, pad)             # second layer: whole 64-channel tiles only
    assert not ops.stem_p3_takes(32, 640, 656, 64, pad)             # 328 output columns: conv_p3 would run strip tiles
    monkeypatch.setattr(ops, 'STEM_P3', False)
    assert not ops.stem_p3_takes(32, 640, 640, 64, pad)


def test_symbol_in_header_and_library():
    from mydetection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'mydet.h')).read()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('mydet_conv_stem_p3_f32', 'mydet_conv_stem_p3_lds_bytes'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', header) and name in _lib.SIGNATURES and hasattr(handle, name)
    assert len(_lib.SIGNATURES['mydet_conv_stem_p3_f32']) == 27
    null = ctypes.c_void_p(0)
    assert _lib.lib().mydet_conv_stem_p3_f32(null, 0, 0, 0, 0, null, null, null, 1, null, null, null, 1, null, 64, 1, 16, 32, 32, 64,
                                             1, 1, 1, 16, 32, 2, null) == -1


def _kernel_resources(substr):
    """{kernel name: registers, scratch and static LDS} of the built library's kernels whose name holds `substr` (code-object metadata)."""
    from mydetection_amd import _lib
    spec = importlib.util.spec_from_file_location('check_store_hazard', os.path.join(ROOT, 'tools', 'check_store_hazard.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    found = {}
    for _, text in mod.code_objects(_lib.LIB_PATH, notes=True):
        if substr not in text:
            continue
        for block in re.split(r'\n\s*-?\s*\.agpr_count:', text)[1:]:      # one block per kernel: .agpr_count is its first key
            name = re.findall(r'\n\s*\.name:\s+(\S+)', block)
            name = [n for n in name if substr in n]
            if not name:
                continue
            field = {k: int(re.search(r'\.' + k + r':\s+(\d+)', block).group(1))
                     for k in ('vgpr_count', 'private_segment_fixed_size', 'group_segment_fixed_size')}
            field['agpr_count'] = int(re.match(r'\s*(\d+)', block).group(1))
            found[name[0]] = field
    return found


def test_kernel_resources_allow_two_workgroups_per_cu():
    import ctypes as ct
    from mydetection_amd import _lib
    if not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('no llvm-readelf on this machine')
    found = _kernel_resources('conv_stem_p3_kernel')
    assert len(found) == 2, found                                       # act NONE and LEAKY
    lds = _lib.lib().mydet_conv_stem_p3_lds_bytes()
    for name, f in found.items():
        assert f['private_segment_fixed_size'] == 0, (name, f)          # no spills
        assert f['vgpr_count'] <= VGPRS_PER_SIMD_LANE // 2, (name, f)   # (vgpr_count includes the accumulation registers) two waves per SIMD
        assert 2 * (f['group_segment_fixed_size'] + lds) <= LDS_PER_CU, (name, f)
    # conv_p3_kernel<S, BN, STRIP, ACT, RES>: stride 1 x {64, 128} x 4 epilogues + stride 2 x {64, 128} x 3 strip forms x 4 epilogues
    found = _kernel_resources('conv_p3_kernel')
    assert len(found) == 32, sorted(found)
    out = (ct.c_int32 * 8)()
    for name, f in found.items():
        S, BN, STRIP = (int(v) for v in re.search(r'conv_p3_kernelILi(\d+)ELi(\d+)ELi(\d+)E', name).groups())
        Wo = 16 + {0: 0, 1: 8, 2: 4}[STRIP]                             # a width that takes the form
        assert _lib.lib().mydet_conv3x3_p3_plan(16, Wo, BN, S, out) == 0 and (out[0], out[1]) == (BN, STRIP), (name, list(out))
        assert f['private_segment_fixed_size'] == 0, (name, f)
        assert f['vgpr_count'] <= VGPRS_PER_SIMD_LANE // 2, (name, f)
        assert 2 * (f['group_segment_fixed_size'] + out[7]) <= LDS_PER_CU, (name, f)
