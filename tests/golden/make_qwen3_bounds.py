"""Write tests/golden/qwen3_bounds.json: the forced ids and the K / V row, tile-maximum and logits
bounds of tests/test_gpu_qwen3.py's decode runs, derived on the CPU as tests/decode_edges_ref.py
derives its own -- 4 x the distance between the fp32- and the fp64-accumulating OracleQwen3
(tests/qwen3_ref.py write_bounds).  No number in it comes from a GPU.

Run:  python tests/golden/make_qwen3_bounds.py      (CPU, under a minute)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"),
                os.path.join(ROOT, "map-reduced-approach-for-vietnamese-long-document-summarization_amd")]

from qwen3_ref import write_bounds  # noqa: E402

if __name__ == "__main__":
    write_bounds()
