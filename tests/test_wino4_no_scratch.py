"""CPU: no instance of the F(4x4) GEMM kernel (csrc/conv_wino4.hip: conv_wino4_kernel<ACT, RES, PART>) uses scratch.

The residual instances used to hold all 16 residual quads beside the 144 accumulators: 256 VGPRs, three 16-byte spills, and a wait
for the residual in front of the last K stage's MFMAs.  The residual is now fetched in two halves of eight quads, so every instance
must report a private segment of 0 in its code-object metadata (read the way tests/test_host_cpu.py::
test_no_kernel_spills_beyond_a_few_registers reads it: tools/check_store_hazard.py)."""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_wino4_gemm_instance_has_no_private_segment():
    from mydetection_amd import _lib
    if not os.path.exists('/opt/rocm/lib/llvm/bin/llvm-readelf'):
        pytest.skip('no llvm-readelf on this machine')
    spec = importlib.util.spec_from_file_location('check_store_hazard', os.path.join(ROOT, 'tools', 'check_store_hazard.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sizes = {}
    for _, text in mod.code_objects(_lib.LIB_PATH, notes=True):
        name = None
        for line in text.splitlines():
            m = re.match(r'\s*\.name:\s+(\S+)', line)
            if m:
                name = m.group(1)
            m = re.match(r'\s*\.private_segment_fixed_size:\s+(\d+)', line)
            if m and name and 'conv_wino4_kernel' in name:
                sizes[name] = int(m.group(1))
    # three activations x {plain, residual} + the K-cut tail's piece instance
    inst = {re.search(r'conv_wino4_kernelILi(\d)ELb([01])ELb([01])E', n).groups() for n in sizes}
    want = {(str(a), r, '0') for a in (0, 1, 2) for r in '01'} | {('0', '0', '1')}
    assert inst == want, sorted(sizes)
    assert all(v == 0 for v in sizes.values()), sizes
