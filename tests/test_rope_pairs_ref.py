"""The relative-position model of tests/test_gpu_rope_pairs.py, its bounds and mutants, recomputed on
the CPU (no GPU, oracle only; tests/rope_pairs_ref.py).

tests/golden/rope_pairs_bounds.json records per config (r3, r8, r1: rope_theta BASE unscaled, prefill GB
3, 2, 1; l3: TINY's llama3-scaled table)
  prefill  the floor per layer (the largest fp32- vs fp64-oracle distance of one hidden row over every
           prompt of the config), the bound (4 x) and every Q mutant's ratio: the whole-row ones
           (position - 1 / + 1, un-rotated, q-block-relative, packed row) and, per pair, the table
           column i ^ 8 and the negated sin;
  decode   (r* only) floors and bounds of decode_edges_ref's observables over the forced sequences, the
           forced ids, the same mutants' ratios on the tile maxima of the decode steps, and the K-side
           twins' ratios on the K rows.
Here all of it is computed again and must
  * meet the conditions: in r3, r8 and r1 every mutant, q_freq(i) and q_conj(i) of each of the 64 pairs
    included, is >= 2 x the bound, once over the prefill hidden rows and once over the decode
    observables, and k_freq(i) / k_conj(i) move the K rows by >= 2 x their bound for all 64 pairs; in
    l3 the whole-row mutants and q_freq(i) / q_conj(i) of every pair of the unscaled band (0..23) and
    of the pairs 29 and 30 of the smoothed band (wavelengths 2048..8192, on the 2048-token prompt) are
    >= 2 x.  The file lists the pairs that reach the ratio ("reached"): 0..31, and 32 for the negated
    sin.  Of the pairs 24..35 tried on the 2048-token prompt, 33, 34 and 35 do not (0.2 - 0.7 x): 35
    and every pair above it is divided by 32 (wavelengths above 2.6e5 tokens), 33 and 34 sit at the
    slow end of the smoothed band (divided by 5.2 and 10) and turn by 0.5 / 0.2 rad in 2048 tokens, and
    q_freq(32) trades a column that turns by 0.9 rad for the still column 40 (0.5 x): out of reach at
    this length;
  * agree with the file: bounds are exactly 4 x the recorded floors, ids equal, every other figure
    within 5 % (two CPU runs under one BLAS: a larger gap means the model or a case changed and the
    file was not rewritten).
"""
import math

import numpy as np
import pytest

import decode_edges_ref as R
import rope_pairs_ref as K
from oracle.llama_ref import _f16, apply_rope, rope_inv_freq, rope_tables

REL = 0.05


def _close(got, want, what):
    assert got == pytest.approx(want, rel=REL), (what, got, want)


def test_constants_come_from_decode_edges():
    assert (K.MARGIN, K.MUTANT_RATIO) == (R.MARGIN, R.MUTANT_RATIO) == (4.0, 2.0)
    assert set(K.golden()["configs"]) == set(K.CONFIGS)
    assert K.P1_LENS == (1, 17, 64, 129, 300, 700) and K.P2_LENS == (1, 17, 64, 129, 65, 1, 320, 128)
    assert K.L3_P1_LENS == (300, 700) and K.L3_LONG == 2048
    assert K.DEC_LENS[:4] == (1, 63, 64, 300) and K.NPRED == 6 and K.DEC_MAX_CTX == 320
    assert max(K.DEC_LENS) + K.NPRED - 1 <= K.DEC_MAX_CTX
    for name in K.CONFIGS:
        for case, lens in K.PREFILL_CASES[name].items():
            ps = K.prefill_prompts(name, case)
            assert [len(p) for p in ps] == list(lens) and all(0 <= p.min() and p.max() < 4000 for p in ps)
    assert [len(p) for p in K.decode_prompts()] == list(K.DEC_LENS)
    assert all(len(f) == K.NPRED - 1 and max(f) < 4000 for f in K.forced_ids())


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_model_is_the_construction(name):
    cfg, w = K.CONFIGS[name], K.weights(name)
    Hq, Hk, D, H = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.hidden
    G = Hq // Hk
    assert K.GB[name] == (3 if G % 3 == 0 else 2 if G % 2 == 0 else 1)  # launch_attn_prefill's choice
    assert H == Hq * D and cfg.n_layers == 2 and (cfg.ffn, cfg.vocab) == (K.TINY.ffn, K.TINY.vocab)
    if name == "l3":
        assert cfg == K.TINY.with_(name=cfg.name)
    else:
        assert cfg.rope_theta == K.BASE and cfg.rope_factor == 0.0
        # the slowest pair turns by more than pi within 300 positions; on TINY's table it turns by 1e-3
        assert 300 * rope_inv_freq(cfg)[63] > math.pi and 300 * rope_inv_freq(K.TINY)[63] < 2e-3
    offs = K.OFFSETS[:Hq]
    assert len(set(offs)) == Hq
    emb = w["embed"]
    assert w["lm_head"] is emb
    assert np.array_equal(emb[:, :K.A], np.tile(emb[:1, :K.A], (cfg.vocab, 1))) and not np.array_equal(emb[7, K.A:], emb[8, K.A:])
    g, theta = K.pair_gains(name, w, K.GAMMA[name], K.CAP), rope_inv_freq(cfg)
    slow = K.L3_SLOW if name == "l3" else 1.0
    assert g.min() > 0 and g.max() <= K.GAMMA[name] * K.CAP * slow
    for ly in w["layers"]:
        assert not ly["wk"][:, K.A:].any() and ly["wk"][:, :K.A].any()
        wq = ly["wq"].reshape(Hq, D, H)
        wk = ly["wk"].reshape(Hk, D, H).astype(np.float64)
        assert np.array_equal(ly["wq"], _f16(ly["wq"]))
        for i in range(K.HALF):
            h = i % Hq
            others = [x for x in range(Hq) if x != h]
            assert not wq[others, i].any() and not wq[others, i + K.HALF].any()
            # the un-rotated query pair is the key pair turned back by d_h positions (+ l3's quarter turn)
            t = offs[h] * theta[i] + (math.pi / 2 if name == "l3" and i >= K.L3_QUARTER else 0.0)
            a, b = wk[h // G, i], wk[h // G, i + K.HALF]
            want = g[i] * np.stack([a * math.cos(t) + b * math.sin(t), b * math.cos(t) - a * math.sin(t)])
            assert np.array_equal(wq[h, [i, i + K.HALF]], _f16(want))


def test_scores_depend_on_relative_position_only():
    """Layer 0 of r3: with the rows' norm factors divided out, q(m) . k(n) is the closed form
    sum_i g_i |z_i|^2 cos((m - n - d_h) theta_i) -- within the fp16 rounding of q and k."""
    name = "r3"
    cfg, w, o = K.CONFIGS[name], K.weights(name), K.oracle(name)
    p = K.main_prompt(name)[:200]
    n, Hq, Hk, D = len(p), cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    raw = {}

    def q_hook(l, q, cos, sin):
        raw.setdefault("q", q)
        return apply_rope(q, cos, sin, _f16)
    cache = o.new_cache()
    o.forward(p, cache, mut={"rope_q": q_hook})
    q = apply_rope(raw["q"], *rope_tables(cfg, np.arange(n)), _f16)
    k = np.repeat(cache["k"][0], Hq // Hk, axis=1)
    s = np.einsum("mhd,nhd->hmn", q.astype(np.float64), k.astype(np.float64))
    z = K.carrier_key(cfg, w)
    zz = z[:, :K.HALF] ** 2 + z[:, K.HALF:] ** 2
    r = np.linalg.norm(cache["k"][0][:, 0].astype(np.float64), axis=-1) / np.linalg.norm(z[0])  # row factor / token 0's
    g, theta = K.pair_gains(name, w, K.GAMMA[name], K.CAP), rope_inv_freq(cfg)
    rel = np.arange(n)[:, None] - np.arange(n)[None, :]
    for h in range(Hq):
        own = np.arange(h, K.HALF, Hq)
        want = sum(g[i] * zz[h // (Hq // Hk), i] * np.cos((rel - K.OFFSETS[h]) * theta[i]) for i in own)
        got = s[h] / (r[:, None] * r[None, :])
        amp = float(sum(g[i] * zz[h // (Hq // Hk), i] for i in own))
        assert np.abs(got - want).max() <= 0.01 * amp, (h, np.abs(got - want).max(), amp)
        assert got.diagonal(-K.OFFSETS[h]).min() >= 0.99 * amp  # the peak sits d_h keys back


def test_rope_q_hook_default_is_unchanged():
    """A ``rope_q`` hook that rotates as the oracle does changes nothing, bit for bit; one that does not
    rotate changes every row but the first."""
    p = K.main_prompt("r3")[:80]
    o = K.oracle("r3")
    base = o.forward(p, collect=True)
    same = o.forward(p, collect=True, mut={"rope_q": lambda l, q, cos, sin: apply_rope(q, cos, sin, _f16)})
    assert np.array_equal(base[0], same[0]) and all(np.array_equal(a, b) for a, b in zip(base[1], same[1]))
    moved = o.forward(p, collect=True, mut=K.q_mutant("r3", "q_unrotated", np.arange(len(p))))
    assert np.array_equal(base[1][0][0], moved[1][0][0])
    assert (R.row_rel(moved[1][0][1:], base[1][0][1:]) > 0).all()
    for kind in K.PAIR_MUTANTS:  # a pair mutant touches its pair's table columns alone
        c0, s0 = rope_tables(K.CONFIGS["r3"], np.arange(5))
        c, s = K._tables(K.CONFIGS["r3"], np.arange(5), kind, 13)
        cols = np.setdiff1d(np.arange(K.HALF), [13])
        assert np.array_equal(c[:, cols], c0[:, cols]) and np.array_equal(s[:, cols], s0[:, cols])
    assert np.array_equal(c[:, 13], c0[:, 13]) and np.array_equal(s[:, 13], -s0[:, 13])


def _check_prefill(name, gp):
    fl = K.prefill_floors(name)
    print(f"{name}: prefill floors", [f"{v:.2e}" for v in fl])
    for l in range(2):
        assert gp["bound"][l] == pytest.approx(K.MARGIN * gp["floor"][l], rel=1e-12)
        _close(fl[l], gp["floor"][l], f"floor layer {l}")
    rows = K.prefill_row_mutants(name, gp["bound"])  # against the RECORDED bounds (what the GPU test asserts)
    print(f"{name}: prefill row mutants", {k: round(v, 1) for k, v in rows.items()})
    assert set(rows) == set(gp["row_mutants"]) >= set(K.ROW_MUTANTS)
    for kind, r in rows.items():
        assert r >= K.MUTANT_RATIO, (kind, r)
        _close(r, gp["row_mutants"][kind], kind)
    return rows


@pytest.mark.parametrize("name", K.RNAMES)
def test_bounds_and_mutants(name):
    gold = K.golden()["configs"][name]
    cfg = K.CONFIGS[name]
    assert (gold["gamma"], gold["cap"], gold["rope_theta"], gold["rope_factor"]) == (K.GAMMA[name], K.CAP, K.BASE, 0.0)
    assert gold["offsets"] == list(K.OFFSETS[:cfg.n_heads])
    gp, gd = gold["prefill"], gold["decode"]
    rows = _check_prefill(name, gp)
    assert "q_pack_row" in rows
    pm = K.prefill_pair_mutants(name, gp["bound"])
    smallest = min(rows.values())
    for kind in K.PAIR_MUTANTS:
        got = [pm[kind][i] for i in range(K.HALF)]
        print(f"{name}: prefill {kind} min {min(got):.1f} (pair {int(np.argmin(got))}) median {np.median(got):.1f}")
        assert len(gp["pair_mutants"][kind]) == K.HALF
        for i in range(K.HALF):
            assert got[i] >= K.MUTANT_RATIO, (kind, i, got[i])
            _close(got[i], gp["pair_mutants"][kind][i], (kind, i))
        smallest = min(smallest, min(got))
    # ---- decode
    assert K.forced_ids() == gd["forced"]
    dfl = K.decode_floors(name)
    print(f"{name}: decode floors", {k: f"{v:.2e}" for k, v in dfl.items()})
    for f in R.FAMILIES:
        assert gd["bound"][f] == pytest.approx(K.MARGIN * gd["floor"][f], rel=1e-12)
        _close(dfl[f], gd["floor"][f], f)
    dm = K.decode_mutants(name, gd["bound"])
    print(f"{name}: decode row mutants", {k: round(dm[k], 1) for k in K.ROW_MUTANTS})
    for kind in K.ROW_MUTANTS:
        assert dm[kind] >= K.MUTANT_RATIO, (kind, dm[kind])
        _close(dm[kind], gd["row_mutants"][kind], kind)
        smallest = min(smallest, dm[kind])
    km = K.k_mutants(name, gd["bound"])
    for kind, got, rec in [(k, dm[k], gd["pair_mutants"][k]) for k in K.PAIR_MUTANTS] + \
                          [(k, km[k], gd["k_mutants"][k]) for k in K.K_MUTANTS]:
        got = [got[i] for i in range(K.HALF)]
        print(f"{name}: decode {kind} min {min(got):.1f} (pair {int(np.argmin(got))}) median {np.median(got):.1f}")
        assert len(rec) == K.HALF
        for i in range(K.HALF):
            assert got[i] >= K.MUTANT_RATIO, (kind, i, got[i])
            _close(got[i], rec[i], (kind, i))
        smallest = min(smallest, min(got))
    print(f"{name}: smallest mutant ratio {smallest:.1f}")


def test_l3_scaled_and_smoothed_bands():
    name = "l3"
    gold = K.golden()["configs"][name]
    gp = gold["prefill"]
    assert "decode" not in gold and (gold["rope_theta"], gold["rope_factor"]) == (500000.0, 32.0)
    # the bands of llama3 scaling at TINY's head_dim: unscaled below wavelength 2048, divided by 32 above 8192
    wl = 2 * math.pi * 500000.0 ** (np.arange(K.HALF) / K.HALF)
    assert (wl[list(K.L3_BANDS["unscaled"])] < 2048).all()
    assert all(2048 <= wl[i] <= 8192 for i in K.L3_BANDS["smoothed"]) and (wl[35:] > 8192).all()
    _check_prefill(name, gp)
    short = K.prefill_pair_mutants(name, gp["bound"], K.L3_BANDS["unscaled"])
    long = K.prefill_pair_mutants(name, gp["bound"], K.L3_LONG_PAIRS, long=True)
    for kind in K.PAIR_MUTANTS:
        got = {**short[kind], **long[kind]}
        print(f"{name}: {kind}", {i: round(r, 1) for i, r in got.items()})
        assert set(gp["pair_mutants"][kind]) == {str(i) for i in got}
        for i in K.L3_BANDS["unscaled"] + K.L3_BANDS["smoothed"]:
            assert got[i] >= K.MUTANT_RATIO, (kind, i, got[i])
        for i, r in got.items():
            rec = gp["pair_mutants"][kind][str(i)]
            if max(r, rec) >= 1.0:  # below the bound a ratio is rounding noise, not a figure
                _close(r, rec, (kind, i))
        reached = [i for i, r in got.items() if r >= K.MUTANT_RATIO]
        assert reached == gp["reached"][kind]
