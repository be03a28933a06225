"""The decisive-key model of tests/test_gpu_attn_keys.py, its bounds, mutants and branch counts,
recomputed on the CPU (no GPU, oracle only; tests/attn_keys_ref.py).

tests/golden/attn_keys_bounds.json records per config (g3, g8, g5, g1: prefill GB 3, 2, 1, 1)
  prefill  the floor per layer (the largest fp32- vs fp64-oracle distance of one hidden row over every
           sequence of P1, P2 and P3), the bound (4 x), per mutant the smallest distance / bound over
           the rows it targets, the smallest distance between two sequences' rows of one pack, and the
           counts of attn_prefill_kernel's lazy-max branches the cases reach in each layer;
  decode   floors and bounds of decode_edges_ref's observables over the four forced sequences, the
           forced ids, and the smallest ratio of a dropped partner key / dropped new token.
Here all of it is computed again and must
  * meet the conditions: every mutant moves every row it targets by >= 2 x the bound (the whole-column
    mutant: at least one row beyond the bound, the count recorded), two sequences' rows differ by
    >= 2 x the bound on every common row, each branch count is >= 1 in each layer of each config, q
    stays far inside fp16;
  * agree with the file: bounds are exactly 4 x the recorded floors, ids equal, every other figure
    within 5 % (two CPU runs under one BLAS: a larger gap means the model or a case changed and the
    file was not rewritten).
"""
import numpy as np
import pytest

import attn_keys_ref as K
import decode_edges_ref as R

REL = 0.05


def test_constants_come_from_decode_edges():
    assert (K.MARGIN, K.MUTANT_RATIO) == (R.MARGIN, R.MUTANT_RATIO)
    assert set(K.golden()["configs"]) == set(K.CONFIGS)


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_model_is_the_construction(name):
    cfg, w = K.CONFIGS[name], K.weights(name)
    G = cfg.n_heads // cfg.n_kv_heads
    assert K.GB[name] == (3 if G % 3 == 0 else 2 if G % 2 == 0 else 1)  # launch_attn_prefill's choice
    assert cfg.hidden == cfg.n_heads * cfg.head_dim and cfg.n_layers == 2
    assert K.still_cos_min(700) >= 0.9999  # 0.99991 at pair 36, position 699
    emb = w["embed"]
    assert w["lm_head"] is emb
    assert np.array_equal(emb[1000:4000, :K.A], np.tile(emb[:1000, :K.A], (3, 1)))
    assert not np.array_equal(emb[7, K.A:], emb[1007, K.A:])
    moving = np.setdiff1d(np.arange(cfg.head_dim), K.STILL)
    for ly in w["layers"]:
        assert not ly["wk"][:, K.A:].any() and ly["wk"][:, :K.A].any()
        wq = ly["wq"].reshape(cfg.n_heads, cfg.head_dim, cfg.hidden)
        wk = ly["wk"].reshape(cfg.n_kv_heads, cfg.head_dim, cfg.hidden)
        assert not wq[:, moving].any()
        for h in range(cfg.n_heads):
            want = (np.float32(K.GAMMA[name]) * wk[h // G, K.STILL]).astype(np.float16).astype(np.float32)
            assert np.array_equal(wq[h, K.STILL], want)
        assert np.array_equal(ly["wq"], ly["wq"].astype(np.float16).astype(np.float32))


def test_plants_are_the_issues():
    """The 700-token prompt: every edge row is in a plant, every partner position of the list is some
    row's hidden key, successors where the list puts them, and no class more than three times."""
    pl = K.plants(700)
    assert pl["succ"] == [63, 127, 128, 191, 255, 575, 698]
    rows = {m for m, _, _ in pl["pairs"]} | set(pl["succ"]) | {s + 1 for s in pl["succ"]}
    assert all(m in rows for x in range(16, 701, 16) for m in (x - 1, x, x + 1) if m <= 699)
    hidden = {k for _, k, _ in pl["pairs"]} | {k for v in pl["co"].values() for k in v}
    assert {0, 63, 64} <= hidden
    assert {"tile_first", "prev_tile_last", "prev", "far"} <= {kind for _, _, kind in pl["pairs"]}
    assert any(m // 64 - k // 64 >= 6 for m, k, _ in pl["pairs"])
    for case, lens in K.PREFILL_CASES.items():
        ps = K.prefill_prompts(case)
        assert [len(p) for p in ps] == list(lens)
        for p in ps:
            assert p.min() >= 0 and p.max() < 4000 and len(set(p.tolist())) == len(p)
            pl = K.plants(len(p))
            nominal = [(m, k) for m, k, _ in pl["pairs"]] + [(s + 1, s) for s in pl["succ"]]
            assert len({m for m, _ in nominal}) == len(nominal)  # no row planted twice
            for m, k in nominal:
                assert k < m and p[m] % 1000 == p[k] % 1000 and p[m] != p[k]
            classes, counts = np.unique(p % 1000, return_counts=True)
            assert counts.max() <= 3
            in_plants = {x for m, k in nominal for x in (m, k)}
            assert all(counts[np.searchsorted(classes, p[i] % 1000)] == 1 for i in range(len(p)) if i not in in_plants)
    assert K.P2_LENS == (1, 17, 64, 129, 65, 1, 320, 128) and K.P3_LENS == (1, 1, 2, 16, 33, 64, 65, 130)
    assert K.P1_LENS == (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 193, 257, 700)


def test_mask_hook_default_is_unchanged():
    """An identity ``mask`` hook changes nothing, bit for bit; a hidden diagonal does."""
    p = K.prefill_prompts("P1")[6]
    o = K.oracle("g3")
    base = o.forward(p, collect=True)
    same = o.forward(p, collect=True, mut={"mask": lambda l, m: m})
    assert np.array_equal(base[0], same[0]) and all(np.array_equal(a, b) for a, b in zip(base[1], same[1]))
    mut, rows = K._mask_mutant("diagonal", len(p))
    assert rows == list(range(1, len(p)))
    moved = o.forward(p, collect=True, mut=mut)
    assert np.array_equal(base[1][0][0], moved[1][0][0]) and not np.array_equal(base[1][0][1], moved[1][0][1])


def _close(got, want, what):
    assert got == pytest.approx(want, rel=REL), (what, got, want)


@pytest.mark.parametrize("name", sorted(K.CONFIGS))
def test_bounds_mutants_and_branches(name):
    gold = K.golden()["configs"][name]
    assert gold["gamma"] == K.GAMMA[name]
    gp, gd = gold["prefill"], gold["decode"]
    # ---- prefill floors and bounds
    fl = K.prefill_floors(name)
    print(f"{name}: prefill floors", [f"{v:.2e}" for v in fl])
    for l in range(2):
        assert gp["bound"][l] == pytest.approx(K.MARGIN * gp["floor"][l], rel=1e-12)
        _close(fl[l], gp["floor"][l], f"floor layer {l}")
    # ---- mutants, scored against the RECORDED bounds (what the GPU test asserts)
    mu = K.prefill_mutants(name, gp["bound"])
    print(f"{name}: prefill mutants", {k: {a: round(b, 1) for a, b in v.items()} for k, v in mu.items()})
    assert set(mu) == set(K.PREFILL_MUTANTS)
    for kind, m in mu.items():
        assert m["rows"] == gp["mutants"][kind]["rows"] and m["rows"] >= 1
        _close(m["ratio"], gp["mutants"][kind]["ratio"], kind)
        if kind == "column":
            assert m["moved"] >= 1
            _close(m["moved"], gp["mutants"][kind]["moved"], "column rows moved")
        else:
            assert m["ratio"] >= K.MUTANT_RATIO, (kind, m)
    sw = K.swapped_ratio(name, gp["bound"])
    assert sw >= K.MUTANT_RATIO
    _close(sw, gp["swapped_ratio"], "swapped sequences")
    # ---- the lazy-max branches, by construction
    br = K.branches(name)
    print(f"{name}: branches", br)
    for layer, b in br.items():
        for k in ("late_grows", "above", "mixed"):
            assert b[k] >= 1, (layer, k)
            _close(b[k], gp["branches"][layer][k], (layer, k))
        assert 0.0 < b["excess"] <= K.LAZY
        _close(b["excess"], gp["branches"][layer]["excess"], (layer, "excess"))
        assert b["qmax"] < 64.0  # fp16 holds 65504
    # ---- decode
    forced = [K.forced_ids(p)[0] for p in K.decode_prompts()]
    assert forced == gd["forced"]
    dfl = K.decode_floors(name)
    print(f"{name}: decode floors", {k: f"{v:.2e}" for k, v in dfl.items()})
    for f in R.FAMILIES:
        assert gd["bound"][f] == pytest.approx(K.MARGIN * gd["floor"][f], rel=1e-12)
        _close(dfl[f], gd["floor"][f], f)
    dm = K.decode_mutants(name, gd["bound"])
    print(f"{name}: decode mutants", {k: round(v, 1) for k, v in dm.items()})
    assert set(dm) == set(K.DEC_MUTANTS)
    for kind, r in dm.items():
        assert r >= K.MUTANT_RATIO, (kind, r)
        _close(r, gd["mutant_ratio"][kind], kind)
    smallest = min([m["ratio"] for k, m in mu.items() if k != "column"] + [sw] + list(dm.values()))
    print(f"{name}: smallest mutant ratio {smallest:.1f}")


def test_decode_partners_are_the_issues():
    """Per sequence the five steps' partners: key 0, key 63, the first key of the last page, none, the
    previous position (clamped to the keys that exist); the 300-key row's new token is always past
    the 256-key split boundary and three of its partners are before it or on it."""
    ps = K.decode_prompts()
    assert tuple(len(p) for p in ps) == K.DEC_LENS == (1, 63, 64, 300) and K.NPRED == 6
    for p in ps:
        fed, partners = K.forced_ids(p)
        n, toks = len(p), p.tolist()
        assert len(fed) == 5 and partners[3] is None and partners[0] == 0
        assert partners[1] == min(63, n) and partners[4] == n + 3
        assert partners[2] == (n + 1) // 64 * 64
        for j, (t, k) in enumerate(zip(fed, partners)):
            if k is None:
                assert all(t % 1000 != x % 1000 for x in toks)
            else:
                assert t % 1000 == toks[k] % 1000 and t not in toks
            toks.append(t)
    fed, partners = K.forced_ids(ps[3])
    split = K.DEC_PPB * 64
    assert partners[:3] == [0, 63, split] and 300 >= split
