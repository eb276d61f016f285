"""GPU: the affinity graphs of many chunks from ONE device call (``ai_affinity_build_batch``).

The oracle is the single build: every chunk of every batched call here is compared, bit for bit in ``indptr``, ``indices`` and
``data``, with ``get_affinity_matrix`` of that chunk alone -- no chunk is left out and nothing is tolerated.  The chunks are the
fixtures of tests/affinity_cases.py, which sit on the thresholds of the kernels (stash, tiles, walk, widths); the groups put
chunk boundaries inside, at and one past a 16-row tile of the weights kernel, chunks that overlap in space next to one that
lies kilometres away, and rows over the stash in none, one or all chunks of a call."""
import numpy as np
import pytest

import affinity_cases as ac

pytestmark = pytest.mark.gpu

MIX = ["walk_line", "walk_sheet", "walk_3d", "walk_3d_negative", "walk_3d_map", "tail_1", "tail_2", "tail_15", "tail_16", "tail_17",
       "tail_31", "tail_32", "tail_33", "tail_1025", "tail_1023"]


def _bits_equal(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and \
        np.array_equal(A.data.view(np.int64), B.data.view(np.int64))


def _trim(f, w):
    """The first w columns of f, zero-padded where f has fewer."""
    if f is None or not w:
        return None
    f = f[:, :w]
    return np.ascontiguousarray(np.concatenate([f, np.zeros((f.shape[0], w - f.shape[1]))], axis=1))


class Chunk:
    """One chunk of a group: a fixture's points with its features at the group's widths."""

    def __init__(self, name, tw, dw):
        c = ac.case(name)
        self.name, self.case = name, c
        self.points = c.points
        self.tarl, self.dino = _trim(c.tarl, tw), _trim(c.dino, dw)
        self.key = (name, tw, dw)


def _group(names, tw, dw, theta, gamma):
    return dict(chunks=[Chunk(n, tw, dw) for n in names], kw=dict(alpha=1.0, theta=theta, gamma=gamma, radius=1.0))


GROUPS = {
    "mix_16_32": lambda: _group(MIX, 16, 32, 0.5, 0.1),
    "dup": lambda: _group(["walk_3d", "walk_3d", "random_mixed"], 16, 32, 0.5, 0.1),
    "ref_widths": lambda: _group(["cliques16", "width_96_384"], 96, 384, 0.5, 0.1),
    "one_over": lambda: _group(["cliques32", "random_mixed"], 32, 48, 0.5, 0.1),
    "none_over": lambda: _group(["cliques_no_row_over", "walk_nx1", "at_radius", "underflow"], 16, 0, 0.5, 0.0),
    "rowwise": lambda: _group(["width_100_112", "width_100_112"], 100, 112, 0.5, 0.1),
    "spatial": lambda: _group(MIX, 0, 0, 0.0, 0.0),
}


@pytest.fixture(scope="module")
def api(ctx):
    from autoinst_amd import ncuts_api
    return ncuts_api


@pytest.fixture(scope="module")
def single(api):
    """``get_affinity_matrix`` of one chunk alone, computed once per (fixture, widths, weights) and shared by every test."""
    memo = {}

    def get(ch, kw):
        k = ch.key + (kw["theta"], kw["gamma"])
        if k not in memo:
            memo[k] = api.get_affinity_matrix(ch.points, ch.tarl, ch.dino, **kw)
        return memo[k]
    return get


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def _batched(api, g, group_rows=None, host=False, order=None):
    """One batched call on the group (device tensors unless `host`); the matrices in the order of ``g['chunks']``."""
    chunks = g["chunks"]
    order = list(range(len(chunks))) if order is None else order
    put = (lambda a: a) if host else _dev
    kw = g["kw"]
    pts = [put(chunks[i].points) for i in order]
    tarl = [put(chunks[i].tarl) for i in order] if kw["theta"] else None
    dino = [put(chunks[i].dino) for i in order] if kw["gamma"] else None
    graphs = api.build_affinity_batch(pts, tarl, dino, group_rows=group_rows, **kw)
    try:
        assert len(graphs) == len(chunks)
        mats = [gr.to_scipy() for gr in graphs]
    finally:
        for gr in graphs:
            gr.free()
    out = [None] * len(chunks)
    for k, i in enumerate(order):
        out[i] = mats[k]
    return out


def _compare(g, mats, single, label):
    for k, (ch, A) in enumerate(zip(g["chunks"], mats)):
        B = single(ch, g["kw"])
        assert A.shape == B.shape, f"[{label}] chunk {k} ({ch.name}): {A.shape[0]} rows for {B.shape[0]}"
        assert _bits_equal(A, B), f"[{label}] chunk {k} ({ch.name}, n {ch.points.shape[0]}) differs from the single build"


def test_mix_puts_chunk_boundaries_inside_at_and_past_a_tile():
    """What the mix claims about itself, from the chunk sizes alone: in the listed order a boundary falls inside and one
    past a 16-row tile of the group (5, 2, 7, 12, 1, ...), in the reversed order one falls at a tile (1023 + 1025 = 2048)."""
    sizes = [ac.case(n).n for n in MIX]
    inner = np.concatenate([np.cumsum(sizes)[:-1], np.cumsum(sizes[::-1])[:-1]]) % 16
    assert (inner == 0).any() and (inner == 1).any() and ((inner > 1) & (inner < 15)).any()
    assert 1 in sizes[1:-1] and sum(sizes) > 1024 and ac.case("tail_1025").n > 1024
    shift = ac.case("walk_3d_map").points.min(0) - ac.case("walk_3d").points.min(0)
    assert np.array_equal(shift, ac.MAP_SHIFT)


@pytest.mark.parametrize("group_rows", [None, 1024, 1])
def test_mix_at_every_group_budget(api, single, group_rows):
    """15 chunks of 16 / 32-d features: walks in one, two and three dimensions that overlap at the origin, the same walk at
    (4e5, 5e6, 2e2), tails around the tile sizes, a one-point chunk in the middle.  Default budget: one group; 1024: tail_1025
    exceeds the budget alone; 1: every chunk its own group."""
    g = GROUPS["mix_16_32"]()
    mats = _batched(api, g, group_rows=group_rows)
    _compare(g, mats, single, f"mix_16_32 group_rows={group_rows}")
    if group_rows is None:
        for ch, A in zip(g["chunks"], mats):   # the independent anchor: the longdouble reference of the fixture
            m = ac.check_affinity(ch.case, A, "batched")
            assert m["max_ratio"] <= 1.0


def test_mix_reversed(api, single):
    g = GROUPS["mix_16_32"]()
    _compare(g, _batched(api, g, order=list(range(len(MIX)))[::-1]), single, "mix_16_32 reversed")


def test_mix_from_numpy_inputs(api, single):
    g = GROUPS["mix_16_32"]()
    _compare(g, _batched(api, g, host=True), single, "mix_16_32 host")
    _compare(g, _batched(api, g, host=True, group_rows=1024), single, "mix_16_32 host group_rows=1024")


def test_concatenated_input_with_offsets(api, single):
    """The other half of the segment convention: one resident tensor per input and the offsets."""
    import torch
    g = GROUPS["mix_16_32"]()
    ch = g["chunks"]
    off = np.cumsum([0] + [c.points.shape[0] for c in ch])
    cat = lambda k: torch.cat([_dev(getattr(c, k)) for c in ch])
    graphs = api.build_affinity_batch(cat("points"), cat("tarl"), cat("dino"), offsets=off, **g["kw"])
    try:
        _compare(g, [gr.to_scipy() for gr in graphs], single, "mix_16_32 offsets")
    finally:
        for gr in graphs:
            gr.free()


@pytest.mark.parametrize("name", ["dup", "ref_widths", "one_over", "none_over", "rowwise", "spatial"])
def test_group(api, single, name):
    """dup: the same cloud twice in one call.  ref_widths (96 / 384): rows over the stash, staged and fallback tiles in both
    chunks.  one_over (32 / 48): rows over the stash in the first chunk only.  none_over (16 / 0): no row over the stash, so no
    second walk; an x extent below one cell, pairs at the radius +- 1 ulp, weights that underflow.  rowwise (100 / 112): the
    wave-per-row path.  spatial: no features at all."""
    g = GROUPS[name]()
    mats = _batched(api, g)
    _compare(g, mats, single, name)
    if name == "dup":
        assert _bits_equal(mats[0], mats[1])
    for rows in (1024, 1):
        _compare(g, _batched(api, g, group_rows=rows), single, f"{name} group_rows={rows}")


# ------------------------------------------------------------------------------------------------ through the cut
@pytest.fixture(scope="module")
def cut_chunks():
    from autoinst_amd import synth
    return [synth.synthetic_chunk(1500, seed=s) for s in range(4)]


def test_batched_graphs_cut_like_single_graphs(api, cut_chunks):
    """Labels and the work of the solve are those of the single builds' graphs: a graph that had lost its points would start
    its segments differently (tests/test_gpu_root_start.py).

    The steps are compared as the device counts them: rows x steps (``spmv_rows``), entries x steps (``spmv_nnz``) and the
    number of solves, each a function of the graphs alone.  ``lanczos_steps`` is not: it counts the launches of a host that
    runs ahead of the asynchronous convergence checks (`ai_flow.inc`: frozen segments take part in a launch without doing work),
    and on an MI355X two cuts of the SAME single-build graphs gave 305 and 294 of them (the batched builds' 298) with every other
    figure equal -- which is why tests/test_gpu_root_start.py compares ``spmv_rows`` between repeats and not the launches.  The single builds'
    graphs are therefore cut twice here, and the batched builds' graphs must give what BOTH of those cuts give."""
    kw = dict(alpha=1.0, theta=0.5, gamma=0.0)
    one = [api.build_affinity(c["points"], c["tarl"], **kw) for c in cut_chunks]
    many = api.build_affinity_batch([c["points"] for c in cut_chunks], [c["tarl"] for c in cut_chunks], **kw)
    runs = []
    try:
        for graphs in (one, one, many):
            labs, ngs, _ = api.ncuts_labels_batch(graphs, T=0.03)
            runs.append((labs, ngs, dict(api.last_stats())))
    finally:
        for gr in one + many:
            gr.free()
    keys = ("lanczos_solves", "null_solves", "spmv_rows", "spmv_nnz", "unconverged")
    for tag, (_, ngs, st) in zip(("single", "single again", "batched"), runs):
        print(f"\n[cut of {tag} builds] groups {ngs} launches {st['lanczos_steps']} " + " ".join(f"{k} {st[k]}" for k in keys))
    (la, na, sa), (la2, na2, sa2), (lb, nb, sb) = runs
    assert na == na2 == nb and all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(la, lb, la2))
    for k in keys:
        assert sa[k] == sa2[k] == sb[k], (k, sa[k], sa2[k], sb[k])
    assert max(na) > 1 and sa["unconverged"] == 0


@pytest.mark.parametrize("builders", [1, 0])
def test_run_chunks_batched_build(cut_chunks, builders):
    from autoinst_amd import sharding
    args = [(c["points"], c["tarl"]) for c in cut_chunks]
    kw = dict(threads=2, batch=3, builders=builders, alpha=1.0, theta=0.5, gamma=0.0, T=0.03)
    want = sharding.run_chunks(args, **kw)
    got = sharding.run_chunks(args, batched_build=True, **kw)
    assert len(got) == len(want) == 4 and all(np.array_equal(a, b) for a, b in zip(got, want))
    # chunks of one batch that do not share their features fall back to the loop
    mixed = [args[0], (cut_chunks[1]["points"], None)]
    kw0 = dict(kw, theta=0.0, batch=2)
    a = sharding.run_chunks(mixed, batched_build=True, **kw0)
    b = sharding.run_chunks(mixed, **kw0)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_handles_are_independent(api, single):
    """Free the middle graph first, cut the first afterwards, export the last."""
    g = _group(["walk_sheet", "walk_3d", "tail_1023"], 16, 32, 0.5, 0.1)
    ch = g["chunks"]
    graphs = api.build_affinity_batch([_dev(c.points) for c in ch], [_dev(c.tarl) for c in ch], [_dev(c.dino) for c in ch], **g["kw"])
    ref = api.build_affinity(ch[0].points, ch[0].tarl, ch[0].dino, **g["kw"])
    try:
        graphs[1].free()
        lab, ng, _ = api.ncuts_labels(graphs[0], graphs[0].n, 0.03)
        want, nw, _ = api.ncuts_labels(ref, ref.n, 0.03)
        assert ng == nw and np.array_equal(lab, want)
        assert _bits_equal(graphs[2].to_scipy(), single(ch[2], g["kw"]))
        assert _bits_equal(graphs[0].to_scipy(), single(ch[0], g["kw"]))
    finally:
        for gr in graphs + [ref]:
            gr.free()


# ------------------------------------------------------------------------------------------------ errors
def _error_calls():
    g = _group(["walk_sheet", "tail_33", "walk_line"], 16, 32, 0.5, 0.1)
    ch = g["chunks"]
    pts, tarl, dino = [c.points for c in ch], [c.tarl for c in ch], [c.dino for c in ch]
    nan = [p.copy() for p in pts]
    nan[1][7, 2] = np.nan
    cat = lambda xs: np.concatenate(xs)
    n = [p.shape[0] for p in pts]
    empty = np.array([0, n[0], n[0], sum(n)])
    back = np.array([0, n[0] + n[1], n[0], sum(n)])
    return g, {
        "nan": (lambda api, **more: api.build_affinity_batch(nan, tarl, dino, **g["kw"], **more), "chunk 1"),
        "empty": (lambda api: api.build_affinity_batch(cat(pts), cat(tarl), cat(dino), offsets=empty, **g["kw"]), "chunk 1"),
        "not_monotone": (lambda api: api.build_affinity_batch(cat(pts), cat(tarl), cat(dino), offsets=back, **g["kw"]), "chunk 1"),
        "theta_without_tarl": (lambda api: api.build_affinity_batch(pts, None, dino, **g["kw"]), "TARL"),
    }


@pytest.mark.parametrize("what", ["nan", "empty", "not_monotone", "theta_without_tarl"])
def test_argument_errors_leave_nothing_behind(api, ctx, single, what):
    """The single build's error type (ValueError), the offending chunk in the message where there is one, no graph left
    registered, and the context builds the right bits afterwards."""
    g, calls = _error_calls()
    call, needle = calls[what]
    before = ctx.mem_info()["graphs_live"]
    with pytest.raises(ValueError, match=needle):
        call(api)
    assert ctx.mem_info()["graphs_live"] == before
    _compare(g, _batched(api, g, host=True), single, f"after {what}")
    assert ctx.mem_info()["graphs_live"] == before


def test_error_in_a_later_group_frees_the_earlier_groups_graphs(api, ctx, single):
    """``group_rows=1`` makes every chunk a group of its own, so chunk 0's graph has been made and registered by an earlier group
    when chunk 1 (a NaN coordinate) is refused: the call's graph owner frees it with the call."""
    g, calls = _error_calls()
    call, needle = calls["nan"]
    before = ctx.mem_info()["graphs_live"]
    with pytest.raises(ValueError, match=needle):
        call(api, group_rows=1)
    assert ctx.mem_info()["graphs_live"] == before
    _compare(g, _batched(api, g, host=True, group_rows=1), single, "after nan in the second group")
    assert ctx.mem_info()["graphs_live"] == before
