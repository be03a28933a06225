"""Register-budget guard for the weight-first gate/up GEMV (CPU: reads the built library's metadata).

The decode step's gate/up projection runs k_gemv.hip gemv_wf_kernel<1, 2, SWIGLU, 3, kXLds, RS>
(issue order 1, the default for that shape) and, under order 2, its kXWave twin.  Like the parent
kernel that tests/test_register_budget.py guards, they stream with two 1024-thread blocks
co-resident per CU, which needs <= 64 VGPRs per lane.
"""
import os

import pytest

from test_isa_order import LIB
from test_register_budget import _kernel_meta

BUDGET = [
    ("_ZN2ms14gemv_wf_kernelILi1ELi2ELi2ELi3ELi1ELb1E", 64),  # gate/up + SwiGLU, deferred norm, block image
    ("_ZN2ms14gemv_wf_kernelILi1ELi2ELi2ELi3ELi1ELb0E", 64),  # plain
    ("_ZN2ms14gemv_wf_kernelILi1ELi2ELi2ELi3ELi3ELb1E", 64),  # per-wave slices
    ("_ZN2ms14gemv_wf_kernelILi1ELi2ELi2ELi3ELi3ELb0E", 64),
]


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmapsum.so not built")
def test_weight_first_gate_up_keeps_two_blocks_per_cu(tmp_path):
    meta = _kernel_meta(tmp_path)
    for prefix, limit in BUDGET:
        hits = [(n, d) for n, d in meta.items() if n.startswith(prefix)]
        assert hits, f"{prefix} not found in the library"
        for n, d in hits:
            assert d["max_flat_workgroup_size"] == 1024, n
            assert d["vgpr_count"] <= limit, f"{n}: {d['vgpr_count']} VGPRs > {limit}"
