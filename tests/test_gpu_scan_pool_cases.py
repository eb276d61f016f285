"""GPU: `ai_scan_pool` (csrc/ai_scanpool.hip) at the kernel limits its hand-made cases leave open.  Fixtures:
tests/scan_pool_cases.py, proven on the CPU by tests/test_scan_pool_cases.py (which also shows which fixture fails for which
wrong rule).

The truth is `scan_pool_ref.pool(case, brute=True)`: counts are exact, means agree within `scan_pool_ref.bound`
(``count * 2^-52 * max|f|``: two float64 sums of the same float32 values in different orders, one division each), a query without
a member has a zero row.  Host arrays, the same call again and resident tensors give the same bits.
"""
import numpy as np
import pytest

import scan_pool_cases as sc
import scan_pool_ref as sp

pytestmark = pytest.mark.gpu


def _run(case, ctx):
    from autoinst_amd import points_api
    return points_api.tarl_pool_map(case["scans"], case["feats"], case["T"], case["chunks"], case["boxes"], case["wins"],
                                    radius=case["radius"], return_count=True, ctx=ctx)


def _check(name, ref, got, cnt):
    assert len(got) == len(ref) == len(cnt), name
    for c, (r, g, n) in enumerate(zip(ref, got, cnt)):
        g, n = np.asarray(g), np.asarray(n)
        assert g.shape == r["mean"].shape and g.dtype == np.float64 and n.dtype == np.int32, (name, c)
        bad = np.flatnonzero(n != r["count"])
        assert bad.size == 0, f"{name}, chunk {c}: {bad.size} counts differ, e.g. query {bad[:5]}: {n[bad[:5]]} vs {r['count'][bad[:5]]}"
        err = np.abs(g - r["mean"])
        assert np.all(err <= sp.bound(r)), f"{name}, chunk {c}: worst excess {np.max(err - sp.bound(r))} at {np.argwhere(~(err <= sp.bound(r)))[:3].tolist()}"
        assert not g[n == 0].any(), (name, c)


@pytest.mark.parametrize("name", sorted(sc.cases()))
def test_fixture_pools_as_brute_force(name, ctx):
    import torch
    case = sc.cases()[name]()
    ref = sp.pool(case, brute=True)
    got, cnt = _run(case, ctx)
    _check(name, ref, got, cnt)
    again, cnt2 = _run(case, ctx)
    dev = {"scans": [torch.from_numpy(s).cuda() for s in case["scans"]], "feats": [torch.from_numpy(f).cuda() for f in case["feats"]],
           "chunks": [torch.from_numpy(q).cuda() for q in case["chunks"]]}
    res, cnt3 = _run({**case, **dev}, ctx)
    for c in range(len(got)):
        assert np.array_equal(again[c], got[c]) and np.array_equal(cnt2[c], cnt[c]), f"{name}: two calls differ in chunk {c}"
        assert np.array_equal(res[c].cpu().numpy(), got[c]) and np.array_equal(cnt3[c].cpu().numpy(), cnt[c]), f"{name}: resident tensors, chunk {c}"


def test_a_key_of_64_bits_is_refused_and_the_context_stays_usable(ctx):
    from autoinst_amd import _ffi
    good = sc.key_bits_case()
    ref = sp.pool(good, brute=True)
    for bits in ((22, 21, 21), (21, 22, 21), (21, 21, 22)):
        case = sc.key_bits_case(bits)
        lay = sc.key_layout(case)
        assert max(lay["bits"]) <= sc.K["AXIS_BITS"] and lay["total"] == 64
        with pytest.raises(ValueError, match=sc.KEY_REFUSAL):
            _run(case, ctx)
        assert sc.KEY_REFUSAL in _ffi.load().ai_last_error().decode("utf-8", "replace")
        got, cnt = _run(good, ctx)
        _check("key_63_bits after a refusal", ref, got, cnt)
