"""CPU proofs for tests/scan_pool_cases.py: every fixture sits in the regime its name claims (tile positions, key bits, run
lengths and widths computed with `scan_pool_ref.cell_of` and the restated bias / bits rule), the model of `ks_flag` and the
pooling equals the brute-force truth on all of them, and three wrong rules are each rejected by the fixtures named for them.
No GPU, no library.  Run with ``-s`` for the figures and the rule -> fixture table."""
import numpy as np
import pytest

import scan_pool_cases as sc
import scan_pool_ref as sp


@pytest.fixture(scope="module")
def built():
    return {name: build() for name, build in sc.cases().items()}


@pytest.fixture(scope="module")
def truth(built):
    return {name: sp.pool(c, brute=True) for name, c in built.items()}


def test_constants_are_read_from_the_sources():
    assert sc.K == dict(SP_TILE=256, LANES=16, WAVE=64, AI_BLOCK=256, NARROW=96, WIDE=384, AXIS_BITS=30, KEY_BITS=63, MAX_INDEX=2.0 ** 30)
    assert sc.TILE_COUNTS == (255, 256, 257, 513) and sc.DIMS == (1, 15, 16, 17, 95, 96, 97, 383, 384) and sc.QUERY_TOTALS == (1, 15, 16, 17)


def test_the_model_and_the_tree_equal_brute_force(built, truth):
    for name, c in built.items():
        assert sc.agrees(sc.pool_model(c), truth[name]), f"{name}: the model of ks_flag / ks_pool misses the rules"
        tree = sp.pool(c)
        assert all(np.array_equal(a["count"], b["count"]) and np.array_equal(a["mean"], b["mean"]) for a, b in zip(tree, truth[name])), name
        assert sum(int(r["count"].sum()) for r in truth[name]) > 0, f"{name}: nothing is pooled"


def test_every_wrong_rule_is_rejected_by_its_fixtures(built, truth):
    table = {}
    for rule in sc.WRONG_RULES:
        table[rule] = [name for name, c in built.items() if not sc.agrees(sc.pool_model(c, rule), truth[name])]
        print(f"{rule:10s} rejected by {', '.join(table[rule])}")
    assert set(sc.REJECTED_BY) == set(sc.WRONG_RULES)
    for rule, names in sc.REJECTED_BY.items():
        assert set(names) <= set(table[rule]), f"{rule}: accepted by {sorted(set(names) - set(table[rule]))}"
    assert all(0 < len(v) < len(built) for v in table.values()), "a wrong rule is accepted everywhere, or tells nothing apart"
    # and where a wrong rule must NOT show: one tile of chunks, one chunk, whole lane steps
    assert set(table["first_tile"]) == set(sc.REJECTED_BY["first_tile"])
    assert not [n for n in table["stop_any"] if len(built[n]["chunks"]) == 1]
    assert not [n for n in table["cut16"] if built[n]["dim"] % sc.LANES == 0] and {"dim_16", "dim_96", "dim_384"} <= set(built)


@pytest.mark.parametrize("n", sc.TILE_COUNTS)
def test_chunk_tile_fixtures(n, built, truth):
    c = built[f"chunk_tiles_{n}"]
    assert len(c["chunks"]) == n and -(-n // sc.TILE) == {255: 1, 256: 1, 257: 2, 513: 3}[n]
    x, s = sc._sources(c)
    inside = np.array([sc._inside(c, b, x, s) for b in range(n)])
    assert (inside.sum(axis=0) == 1).all(), "disjoint boxes: every source is inside one chunk only"
    owner = inside.argmax(axis=0)
    m0 = c["scans"][0].shape[0]
    assert np.array_equal(owner[:m0], c["owner0"])
    last, other = n - 1, min(sc.TILE, n - 1)
    first_wave, second_wave = owner[:64].tolist(), owner[64:128].tolist()
    assert first_wave == [0] * 63 + [last] and second_wave == [0] * 32 + [other] * 32
    assert last % sc.TILE == {255: 254, 256: 255, 257: 0, 513: 0}[n], "the last record's place in its tile"
    if n > sc.TILE:
        assert other == sc.TILE and other % sc.TILE == 0, "placed by the first record of the second tile only"
        assert (owner == sc.TILE - 1).sum() >= 2, "and sources placed by the last record of the first tile only"
    assert all((r["count"] > 0).all() for r in truth[c["name"]]), "every query of every chunk has members"
    assert not sc.flag_model(c, "stop_any")[63] and sc.flag_model(c)[63]
    print(f"chunk_tiles_{n}: {x.shape[0]} sources, {sum(q.shape[0] for q in c['chunks'])} queries, {-(-n // sc.TILE)} tiles")


def test_width_and_query_tail_fixtures(built, truth):
    for d in sc.DIMS:
        c = built[f"dim_{d}"]
        assert c["dim"] == d and all(f.shape[1] == d for f in c["feats"]) and c["chunks"][0].shape[0] == sc.LANES + 1
        assert truth[c["name"]][0]["count"].max() > 1
    assert [(d <= sc.NARROW, -(-d // sc.LANES), d % sc.LANES) for d in sc.DIMS] == [
        (True, 1, 1), (True, 1, 15), (True, 1, 0), (True, 2, 1), (True, 6, 15), (True, 6, 0), (False, 7, 1), (False, 24, 15), (False, 24, 0)]
    for t in sc.QUERY_TOTALS:
        for k in (1, 3):
            c = built[f"query_tail_{t}_over_{k}"]
            sizes = [q.shape[0] for q in c["chunks"]]
            assert len(sizes) == k and sum(sizes) == t
            assert sizes == ([t] if k == 1 else [0, 1, 0] if t == 1 else [t // 3 + (1 if i < t % 3 else 0) for i in range(3)])
            assert -(-t * sc.LANES // sc.K["AI_BLOCK"]) == (2 if t > 16 else 1)


def test_empty_end_scans_fixture(built, truth):
    c = built["empty_end_scans"]
    assert [s.shape[0] for s in c["scans"]] == [0, 100, 100, 100, 0]
    assert c["wins"].tolist() == [[0, 5], [1, 4], [0, 2], [3, 5]]
    t = truth["empty_end_scans"]
    both = sp.pool({**c, "chunks": [c["chunks"][0]] * 2, "boxes": c["boxes"][:2], "wins": c["wins"][:2]}, brute=True)
    assert np.array_equal(both[0]["count"], both[1]["count"]) and both[0]["count"].sum() > 0, "an empty scan adds nothing to a window"
    assert t[2]["count"].sum() > 0 and t[3]["count"].sum() > 0
    # segment_of on offsets with empty segments at both ends: the scan of point i is the last s with off[s] <= i
    off = np.concatenate([[0], np.cumsum([s.shape[0] for s in c["scans"]])])
    assert off.tolist() == [0, 0, 100, 200, 300, 300]
    seg = np.searchsorted(off, np.arange(300), side="right") - 1
    assert seg.min() == 1 and seg.max() == 3 and np.array_equal(seg, sc._sources(c)[1])


def test_key_bit_fixtures(built, truth):
    c = built["key_63_bits"]
    lay = sc.key_layout(c)
    assert lay["bits"] == [21, 21, 21] and lay["total"] == sc.K["KEY_BITS"] and lay["refused"] is None
    assert all(b < 0 for b in lay["bias"])
    x, _ = sc._sources(c)
    idx = sp.cell_of(x)
    assert (idx.min(axis=0) < -(1 << 19)).all() and (idx.max(axis=0) > (1 << 19)).all(), "negative and positive cell indices"
    rel = idx - np.array(lay["bias"])
    assert (rel >= 0).all() and (rel < (1 << 21)).all() and (rel.max(axis=0) > (1 << 21) - 64).all(), "the fields are used to their ends"
    assert all(r["count"].sum() > 0 for r in truth["key_63_bits"]), "both corners pool"
    wide = sc.key_layout(sc.key_bits_case((22, 21, 21)))
    assert wide["bits"] == [22, 21, 21] and max(wide["bits"]) <= sc.K["AXIS_BITS"] and wide["total"] == 64 and wide["refused"] == "key"
    for bits in ((21, 22, 21), (21, 21, 22)):
        assert sc.key_layout(sc.key_bits_case(bits))["refused"] == "key"
    print(f"key_63_bits: bias {lay['bias']}, bits {lay['bits']}; 22 + 21 + 21 is refused")
