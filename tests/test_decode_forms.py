"""The decode regime table on the CPU: which kernel family and split each decode projection of a
Llama-3.2-3B engine launches, per engine size and weight type.

pick_form (csrc/decode_forms.h) is the one function that ranks the kernel families, over plain
data and the launchers' *_supported predicates -- host code that needs no device.  The standalone
tests/native/decode_forms.cpp asks it with the engine's own calls and compares the answers with
its table; this test links that program against the built objects (`make forms`) and runs it.

The same program sweeps the decode-attention workspaces: every split grid decode_run can launch
(decode_forms.h decode_grid_len: rounded up to 256 keys, past max_ctx when that is no multiple of
256) against the bytes and the partial stride ms_create allocates, for every MS_ATTN_PPB /
MS_ATTN_PPW setting, engine shape, reachable context length and run length.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd", "csrc")
LIB = os.path.join(os.path.dirname(CSRC), "mapsum", "libmapsum.so")
BIN = os.path.join(ROOT, "tests", "native", "decode_forms")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmapsum.so not built")
def test_decode_regime_table():
    subprocess.run(["make", "-C", CSRC, "-j", "16", "forms"], check=True, capture_output=True, timeout=1200)
    # the table is the defaults': no tuning variable of the caller's reaches resolve_settings
    env = {k: v for k, v in os.environ.items() if not k.startswith(("MS_", "MAPSUM_"))}
    r = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=60)
    print(r.stdout)
    print(r.stderr[-3000:])
    assert r.returncode == 0 and "DECODE_FORMS_OK" in r.stdout
    assert "workspace sweep:" in r.stdout and " 0 engine shapes too small" in r.stdout
