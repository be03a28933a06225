"""The bounds of tests/test_gpu_decode_edges.py, recomputed on the CPU (no GPU, oracle only).

tests/golden/decode_edges_bounds.json records, per case, the noise floor of every observable
family (fp32- vs fp64-accumulating oracle, tests/decode_edges_ref.py), the bound (4 x the floor)
the GPU test asserts, and the smallest ratio distance / bound of every kind of deliberately wrong
reference.  Here the floors and the mutants are computed again and must
  * leave every mutant of every case at >= 2 x the bound on an observable the case asserts --
    scored on nothing the GPU test of that case does not read: f has no pool rows, g the partials
    of every third step only -- (a mutant: one fault in one sequence, at every step; with every
    single step a mutant of its own, all kinds but the swapped V rows and f's unreadable rows
    still hold 2 x), and
  * agree with the file: the bounds are exactly 4 x the recorded floors; a recomputed floor lies
    within 25 % of the recorded one (it is the largest of 60-240 samples of summation-order noise,
    and the fp32 sums follow the BLAS build of the machine); a recomputed mutant ratio within 10 %
    (a mutant moves the observables by 2-500 x the bound, the noise by <= 1/4 of it).
"""
import numpy as np
import pytest

import decode_edges_ref as R
from mapsum.config import TINY
from oracle.llama_ref import OracleLlama
from oracle.synth import make_weights


def test_cases_are_the_issues():
    """Every slot filled, the longest sequence last, generation inside max_ctx."""
    for name, c in R.CASES.items():
        assert len(c["lens"]) == c["max_batch"], name
        assert c["lens"][-1] == max(c["lens"]) and c["lens"][-1] + R.NPRED <= c["max_ctx"], name
    assert R.CASES["a"]["lens"][-1] + R.NPRED == R.CASES["a"]["max_ctx"]  # ends at exactly max_ctx
    assert R.CASES["d"]["max_ctx"] % R.PAGE != 0
    assert set(R.golden()["cases"]) == set(R.CASES)


def test_oracle_accumulation_dtype():
    """acc=float32 is the default, and an empty ``mut`` changes nothing (that the default still
    computes what it did before ``acc`` existed is shown by the goldens of tests/test_oracle.py,
    not here); float64 keeps the rounding points, so it stays within the contract's rounding noise
    of the default without being identical."""
    w = make_weights(TINY, R.SEED, std=R.STD, jitter=R.JITTER)
    ids = np.random.default_rng(5).integers(0, 4000, size=70)
    base, _ = OracleLlama(TINY, w).forward(ids)
    same, _ = R.oracle().forward(ids, mut={})
    wide, _ = R.oracle(np.float64).forward(ids)
    assert np.array_equal(base, same)
    assert wide.dtype == np.float32 and 0 < R.rel(wide, base) < 2e-3
    with pytest.raises(AssertionError):
        OracleLlama(TINY, w, acc=np.float16)


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_bounds_and_mutants(case):
    gold = R.golden()["cases"][case]
    for f in R.FAMILIES:
        assert gold["bound"][f] == pytest.approx(R.MARGIN * gold["floor"][f], rel=1e-12), f
    fl = R.floors(case)
    print("floors", {k: f"{v:.2e}" for k, v in fl.items()})
    for f, v in fl.items():
        assert 0.75 * gold["floor"][f] <= v <= 1.25 * gold["floor"][f], (f, v, gold["floor"][f])
    # layer 0's K / V come straight from the embedding row through one GEMM: nearly exact
    assert fl["k_layer0"] < fl["k"] and fl["v_layer0"] < fl["v"]
    ratios = R.mutant_ratios(case, gold["bound"])
    print("mutant ratios", {k: round(v, 2) for k, v in ratios.items()})
    longest = R.CASES[case]["lens"][-1] + R.NPRED - 1
    want = set(R.MUTANT_KINDS)
    if min(R.CASES[case]["split_keys"]) >= longest:
        want.discard("drop_split_first")  # one split: no boundary below the longest context
    assert set(ratios) == want
    for kind, r in ratios.items():
        assert r >= R.MUTANT_RATIO, (kind, r)
        assert r == pytest.approx(gold["mutant_ratio"][kind], rel=0.1), kind
    # stricter: every single step whose logits observable the case reads a mutant of its own; the
    # two exceptions are explained in decode_edges_ref.mutant_ratios
    steps = R.mutant_ratios(case, gold["bound"], per_step=True)
    print("per step", {k: round(v, 2) for k, v in steps.items()})
    assert set(steps) == want
    for kind, r in steps.items():
        assert r == pytest.approx(gold["mutant_ratio_step"][kind], rel=0.1), kind
        unreadable = kind in R.WRITE_KINDS and not R.CASES[case]["pools"]
        assert kind == "swap_v" or unreadable or r >= R.MUTANT_RATIO, (kind, r)
