"""Register-budget guard for the line-exact gate/up GEMVs (CPU: reads the built library's metadata).

k_gemv.hip gemv_lx_kernel<1, 2, SWIGLU, 3, XM, RS, WF, LX> loads the weights line-exact and swaps
half-rows between lanes before each MFMA step (gemv_common.h lx_exchange).  Like the pair-form
kernels that tests/test_register_budget.py and tests/test_gemv_order_budget.py guard, it streams
with two 1024-thread blocks co-resident per CU, which needs <= 64 VGPRs per lane: the exchange's
temporaries and the X fragments are kept from being live together (66 VGPRs otherwise).
"""
import os

import pytest

from test_isa_order import LIB
from test_register_budget import _kernel_meta

PREFIX = "_ZN2ms14gemv_lx_kernelILi1ELi2ELi2ELi3E"  # every X mode, issue order, policy, with / without row scale


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmapsum.so not built")
def test_line_exact_gate_up_keeps_two_blocks_per_cu(tmp_path):
    meta = _kernel_meta(tmp_path)
    hits = [(n, d) for n, d in meta.items() if n.startswith(PREFIX)]
    assert len(hits) == 12, f"expected 3 issue forms x 2 policies x 2 row-scale variants, found {len(hits)}"
    for n, d in hits:
        assert d["max_flat_workgroup_size"] == 1024, n
        assert d["vgpr_count"] <= 64, f"{n}: {d['vgpr_count']} VGPRs > 64"
