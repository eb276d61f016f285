"""GPU: both affinity builds at their grid limits, the batched build at the thresholds of its groups (fixtures and host model:
tests/affinity_batch_cases.py; that every fixture sits on its threshold is proven on the CPU in
tests/test_affinity_batch_cases.py).

Oracles.  Every chunk of every batched call is compared with ``get_affinity_matrix`` of that chunk alone: ``indptr``,
``indices`` and the bits of ``data`` are equal, nothing is tolerated and no chunk is left out.  The single build, and once per
fixture the batched one (`Call.anchors`), also goes through `affinity_cases.check_affinity`: the pattern of the float64
predicate, values within the derived bound of the ``np.longdouble`` ones, ``max_ratio <= 1.0``.

The calls that need cell tables of 2^28 cells (2.1 GB) run on a `Context` of their own, closed with the module, so that the
session's default context does not keep that workspace."""
import re
import time

import numpy as np
import pytest

import affinity_batch_cases as bc
import affinity_cases as ac

pytestmark = pytest.mark.gpu


def _bits_equal(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and \
        np.array_equal(A.data.view(np.int64), B.data.view(np.int64))


@pytest.fixture(scope="module")
def api(ctx):
    from autoinst_amd import ncuts_api
    return ncuts_api


@pytest.fixture(scope="module")
def big_ctx(api):
    c = api.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def single(api):
    """``get_affinity_matrix`` of one chunk alone, once per (chunk, weights), shared by every test and left unchanged."""
    memo = {}

    def get(ch, call, ctx):
        k = (id(ch), call.theta, call.gamma)
        if k not in memo:
            memo[k] = api.get_affinity_matrix(ch.points, ch.tarl if call.theta else None, ch.dino if call.gamma else None, ctx=ctx, **call.kw)
        return memo[k]
    return get


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).cuda()


def _batched(api, call, ctx, host=False):
    """The call's chunks through ONE ``build_affinity_batch``: the exported matrices, in the caller's order."""
    put = (lambda a: a) if host else _dev
    pts = [put(c.points) for c in call.chunks]
    tarl = [put(c.tarl) for c in call.chunks] if call.theta else None
    dino = [put(c.dino) for c in call.chunks] if call.gamma else None
    graphs = api.build_affinity_batch(pts, tarl, dino, group_rows=call.group_rows, ctx=ctx, **call.kw)
    try:
        assert len(graphs) == len(call.chunks)
        return [g.to_scipy() for g in graphs]
    finally:
        for g in graphs:
            g.free()


def _compare(call, mats, single, ctx):
    for k, (ch, A) in enumerate(zip(call.chunks, mats)):
        B = single(ch, call, ctx)
        assert A.shape == B.shape, f"[{call.name}] chunk {k} ({ch.name}): {A.shape[0]} rows for {B.shape[0]}"
        assert _bits_equal(A, B), f"[{call.name}] chunk {k} ({ch.name}, n {ch.n}) differs from the single build"
    for k in call.anchors:
        m = ac.check_affinity(call.chunks[k].case(call.theta, call.gamma), mats[k], f"{call.name} chunk {k}")
        assert m["max_ratio"] <= 1.0


def _builds(api, single, ctx, name, host=False):
    call = bc.call(name)
    assert call.error is None
    t0 = time.perf_counter()
    mats = _batched(api, call, ctx, host)
    dt = time.perf_counter() - t0
    _compare(call, mats, single, ctx)
    print(f"\n[{name}] {len(call.chunks)} chunks, {sum(c.n for c in call.chunks)} rows: batched build and export {dt:.3f} s")
    return mats


def _refused(api, ctx, name, host=True):
    """The call raises ValueError naming its chunk and the limit, and leaves no graph behind."""
    call = bc.call(name)
    chunk, why = call.error
    before = ctx.mem_info()["graphs_live"]
    with pytest.raises(ValueError, match=rf"chunk {chunk}\b.*{re.escape(bc.MESSAGE[why])}"):
        _batched(api, call, ctx, host)
    assert ctx.mem_info()["graphs_live"] == before


# ------------------------------------------------------------------------------------------------- 1. the axis limit
@pytest.mark.parametrize("name", bc.LINE_NAMES)
def test_axis_limit_single_build(api, ctx, name):
    """1023 cells on one axis, the last point in cell 1022 (bit 9 of the coordinate: bit 27, 28 or 29 of the Morton key); one
    double further the build refuses."""
    ch = bc.call(name).chunks[0]
    m = ac.check_affinity(ch.case(0.0, 0.0), api.get_affinity_matrix(ch.points, alpha=1.0, theta=0.0, gamma=0.0, radius=1.0), "single")
    assert m["max_ratio"] <= 1.0
    over = bc.call(name + "_over").chunks[1]
    with pytest.raises(ValueError, match="1023 cells per axis"):
        api.get_affinity_matrix(over.points, alpha=1.0, theta=0.0, gamma=0.0, radius=1.0)


@pytest.mark.parametrize("name", bc.LINE_NAMES)
def test_axis_limit_batched_build(api, ctx, single, name):
    _builds(api, single, ctx, name)
    _refused(api, ctx, name + "_over")


# ------------------------------------------------------------------------------------------------- 2. the cell limit
def test_cell_limit_single_build(api, big_ctx):
    """1023 x 512 x 512 = 268 173 312 cells, a cluster in each corner cell: cell 268 173 311 is the largest a table ever holds."""
    ch = bc.cells_at_limit()
    A = api.get_affinity_matrix(ch.points, alpha=1.0, theta=0.0, gamma=0.0, radius=1.0, ctx=big_ctx)
    assert ac.check_affinity(ch.case(0.0, 0.0), A, "single")["max_ratio"] <= 1.0
    with pytest.raises(ValueError, match="dense cell-table limit"):
        api.get_affinity_matrix(bc.cells_over().points, alpha=1.0, theta=0.0, gamma=0.0, radius=1.0, ctx=big_ctx)


def test_cell_limit_batched_build(api, big_ctx, single):
    _builds(api, single, big_ctx, "cells_at_limit")
    _refused(api, big_ctx, "cells_over")
    _refused(api, big_ctx, "cells_over_in_the_middle")


# ------------------------------------------------------------------------------------------------- 3. chunk counts
@pytest.mark.parametrize("nc", bc.CHUNK_COUNTS)
def test_chunk_counts(api, ctx, single, nc):
    """One group of nc chunks of 1 .. 40 rows that all lie in one another's space, 16 / 32-d features: the key width changes from
    16 to 17 and from 256 to 257 chunks, `k_b_chunk_entries` takes its second block from 256 chunks.  In the 17- and 257-chunk
    groups chunk 0 is `long_x` and the last chunk `long_z`: bit 29 of the Morton key directly under the top bit of the chunk id."""
    _builds(api, single, ctx, f"chunks_{nc}")


# ------------------------------------------------------------------------------------------------- 4. the split
@pytest.mark.parametrize("name", ["split_pair", "split_control", "split_three", "split_five", "split_deep", "split_second_group"])
def test_split(api, big_ctx, single, name):
    """Groups whose chunks ask for more than 2^28 cells together are redone as their halves (`Call.built` / `Call.split`, proven
    on the CPU); every chunk equals its single build, in the caller's order."""
    _builds(api, single, big_ctx, name, host=(name == "split_five"))


def test_the_split_really_happens(api):
    """The workspace a fresh context holds after the call -- derived, not measured.  The arena takes a block of exactly the
    size asked for when that is above 256 MB, and of 256 MB otherwise.  `split_control` (2^28 cells in one group) needs its two
    int32 cell tables at once: at least 2 * 4 * 2^28 bytes.  `split_pair` never holds more than the tables of its larger half,
    which is built first: 256 MB for the small buffers before the tables, 2 * 4 * 513 * 2^18 bytes of tables, 256 MB for the small
    buffers after them -- the second half's tables (2 * 4 * 2^27) fit the same blocks -- 1 612 709 888 bytes, below 2^31."""
    info = {}
    for name in ("split_pair", "split_control"):
        c = api.Context()
        try:
            call = bc.call(name)
            graphs = api.build_affinity_batch([x.points for x in call.chunks], [x.tarl for x in call.chunks] if call.theta else None,
                                              [x.dino for x in call.chunks] if call.gamma else None, ctx=c, **call.kw)
            info[name] = c.mem_info()["workspace"]
            for g in graphs:
                g.free()
        finally:
            c.close()
    print(f"\nworkspace after split_pair {info['split_pair']} B, after split_control {info['split_control']} B")
    assert info["split_pair"] < 2 ** 28 * 8
    assert info["split_control"] >= 2 ** 28 * 8


def test_split_then_error(api, big_ctx, single):
    """A group that splits and is built, then a group whose chunk has a NaN coordinate: the call names that chunk, frees the
    graphs of the halves, and the next call builds the right bits."""
    before = big_ctx.mem_info()["graphs_live"]
    _refused(api, big_ctx, "split_then_error")
    _builds(api, single, big_ctx, "split_pair")
    assert big_ctx.mem_info()["graphs_live"] == before


# ------------------------------------------------------------------------------------------------- 5. k_b_bounds
@pytest.mark.parametrize("n", bc.BOUNDS_NS)
def test_bounds_with_several_blocks(api, ctx, single, n):
    """A chunk of n rows between a one-point chunk and one of 300: S = 1, 2, 3 blocks of `k_b_bounds` per chunk.  The points that
    alone carry the minimum and the maximum (the axis limit itself) of x sit in rows that only the last block reads, on the last
    trip of its threads 0 and 255."""
    _builds(api, single, ctx, f"bounds_{n}")


@pytest.mark.parametrize("variant", bc.BOUNDS_VARIANTS[1:])
@pytest.mark.parametrize("n", bc.BOUNDS_NS)
def test_bounds_refuse_what_only_the_last_block_sees(api, ctx, n, variant):
    """The same chunk with that one row a double over the axis limit, or holding a NaN, +inf or -inf."""
    _refused(api, ctx, f"bounds_{n}_{variant}")
    _refused(api, ctx, f"bounds_{n}_{variant}", host=False)


def _lattice_reference():
    """Pattern and value of the lattice's graph, from the lattice itself: a point's neighbours are the six one step (0.75) along
    an axis -- the diagonal ones are 1.06 away -- in ascending order of their ids."""
    nx, ny, nz = bc.LATTICE
    ix, iy, iz = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    r = ((ix * ny + iy) * nz + iz).reshape(-1)
    ok = [ix > 0, iy > 0, iz > 0, np.ones_like(ix, dtype=bool), iz < nz - 1, iy < ny - 1, ix < nx - 1]
    step = [-ny * nz, -nz, -1, 0, 1, nz, ny * nz]
    mask = np.stack([m.reshape(-1) for m in ok], axis=1)
    cand = r[:, None] + np.array(step)[None, :]
    return np.concatenate([[0], np.cumsum(mask.sum(1))]), cand[mask], np.broadcast_to(np.array(step) == 0, mask.shape)[mask]


def test_bounds_cap(api, ctx, single):
    """A lattice of 102 x 101 x 102 points (1 050 804 rows, 7 entries per inner row) beside a 300-point chunk: S at its cap of 256,
    16 or 17 trips per thread.  The one large case: the batched build with its export took 0.011 s and the whole test, with the
    single build of the lattice and the comparisons, 0.16 s on an MI355X."""
    mats = _builds(api, single, ctx, "bounds_cap")
    indptr, indices, diag = _lattice_reference()
    A = mats[1]
    assert np.array_equal(A.indptr, indptr) and np.array_equal(A.indices, indices)
    want = np.exp(-ac.LD(1.0) * ac.LD(bc.LATTICE_STEP))
    err = np.abs(A.data[~diag].astype(ac.LD) - want).astype(np.float64)
    assert (A.data[diag] == 1.0).all() and err.max() <= ac._factor_err(bc.LATTICE_STEP, 3) * float(want) + ac.TINY


# ------------------------------------------------------------------------------------------------- 6. the chunk cap
@pytest.mark.parametrize("nan_at", [0, 65534])
def test_more_chunks_than_a_grid_has_rows(api, ctx, single, nan_at):
    """65 536 one-point chunks: groups of 65 535 (the `y` limit of a launch) and 1.  A NaN in the first or in the last chunk of the
    first group ends the call in that group's bounds pass, before any graph is made."""
    p, off = bc.many_chunks(nan_at=nan_at)
    before = ctx.mem_info()["graphs_live"]
    with pytest.raises(ValueError, match=rf"chunk {nan_at}\b.*not finite"):
        api.build_affinity_batch(p, offsets=off, alpha=1.0, theta=0.0, gamma=0.0, radius=1.0)
    assert ctx.mem_info()["graphs_live"] == before
    _builds(api, single, ctx, "chunks_3")
    assert ctx.mem_info()["graphs_live"] == before
