"""The decode regime table at the Qwen3-8B widths (hidden 4096, ffn 12288), on the CPU.

The default split-K counts are tuned for K = 3072 / 8192; 6 does not divide 4096 in whole 64-k
steps, and the K-quant skinny GEMM wants K / (256 S) even or a multiple of 3.  The standalone
tests/native/decode_forms_qwen3.cpp asks pick_form (csrc/decode_forms.h) as the engine asks it, for
fp16 and Q4_K_M engines of 8 / 20 / 32 / 128 / 256 slots at EVERY row count 1 .. max_batch: each
projection must resolve to a real kernel family with a split its launcher accepts, the same at every
row count of one engine.  Built and run the way tests/test_decode_forms.py runs its driver.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd", "csrc")
LIB = os.path.join(os.path.dirname(CSRC), "mapsum", "libmapsum.so")
BIN = os.path.join(ROOT, "tests", "native", "decode_forms_qwen3")


@pytest.mark.skipif(not os.path.exists(LIB), reason="libmapsum.so not built")
def test_qwen3_decode_forms_resolve():
    subprocess.run(["make", "-C", CSRC, "-j", "16", "forms"], check=True, capture_output=True, timeout=1200)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("MS_", "MAPSUM_"))}
    r = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    print(r.stderr[-3000:])
    assert r.returncode == 0 and "QWEN3_FORMS_OK" in r.stdout
