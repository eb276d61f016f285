"""CPU proofs for tests/affinity_batch_cases.py: every fixture sits on the threshold its name says -- cell counts, Morton bits,
the blocks of `k_b_bounds` and the rows of the extreme points, the group plans, the chunk cap -- and each wrong variant of the
host model changes the plan or the expected result of the fixtures named for it.  No GPU, no library.  Run with ``-s`` to see
the variant -> fixture table."""
import numpy as np
import pytest

import affinity_batch_cases as bc
import affinity_cases as ac


# ------------------------------------------------------------------------------------------------- the model of the grid
def test_constants():
    assert (bc.AI_BLOCK, bc.BOUNDS_ROWS, bc.BOUNDS_MAX_BLOCKS, bc.KEY_BITS) == (256, 4096, 256, 30)
    assert (bc.CELL_LIMIT, bc.DEFAULT_GROUP_ROWS, bc.MAX_ROWS, bc.MAX_GROUP_CHUNKS) == (2 ** 28, 2 ** 21, 2 ** 30, 65535)
    assert [bc.bits_for(k) for k in (0, 1, 2, 3, 4, 5, 16, 17, 256, 257)] == [0, 0, 1, 2, 2, 3, 4, 5, 8, 9]


@pytest.mark.parametrize("name", ["walk_3d", "walk_3d_map", "walk_nx1", "tail_1", "random_mixed"])
def test_affinity_grid_is_grid_of_where_nothing_is_refused(name):
    p = ac.case(name).points
    why, dims, ncell = bc.single_grid(p)
    assert why == bc.OK and dims == ac.grid_of(p, 1.0)[2] and ncell == dims[0] * dims[1] * dims[2]
    S, w, cells, d = bc.group_boxes(p, [0, p.shape[0]], 0, 1)
    assert w.tolist() == [0] and cells.tolist() == [ncell] and tuple(d[0]) == dims


def test_refusals_of_the_grid():
    assert bc.affinity_grid([0, 0, 0], [1, np.inf, 1])[0] == bc.NOT_FINITE
    assert bc.affinity_grid([0, 0, 0], [1e15, 1, 1])[0] == bc.NOT_FINITE
    assert bc.affinity_grid([1e300] * 3, [-1e300] * 3)[0] == bc.NOT_FINITE          # what a cloud of NaN leaves of the fold
    assert bc.affinity_grid([0, 0, 0], [1, 1023.5, 1])[0] == bc.AXIS
    assert bc.affinity_grid([0, 0, 0], [1022.5, 512.5, 511.5])[0] == bc.CELLS


# ------------------------------------------------------------------------------------------------- 1. the axis limit
@pytest.mark.parametrize("name", bc.LINE_NAMES)
def test_lines_end_on_the_last_double_of_the_axis(name):
    c, over = bc.call(name), bc.call(name + "_over")
    p, q = c.chunks[0].points, over.chunks[1].points
    a = "xyz".index(name[5])
    cell = 1.0 * (1.0 + 1e-9)
    mn, top = p[:, a].min(), p[:, a].max()
    assert np.array_equal(p.min(0), ac.MAP_SHIFT if name.endswith("_map") else np.zeros(3))
    assert top == p[-1, a] == bc.axis_limit(mn) and (top - mn) / cell < 1023.0 <= (np.nextafter(top, np.inf) - mn) / cell
    assert q[-1, a] == np.nextafter(top, np.inf) and np.array_equal(p[:-1], q[:-1]) and np.array_equal(np.delete(p, a, 1), np.delete(q, a, 1))
    assert p.shape[0] == 2047 and np.all(np.diff(p[:-1, a]) == 0.5) and 0.5 < top - p[-2, a] <= 1.0      # the last point has a neighbour
    why, dims, ncell = bc.single_grid(p)
    want = [1, 1, 1]
    want[a] = 1023
    assert why == bc.OK and list(dims) == want == list(ac.grid_of(p, 1.0)[2]) and ncell == 1023
    cells = ac.grid_of(p, 1.0)[3]
    assert cells[-1, a] == 1022 == cells[:, a].max()
    key = int(ac.morton_keys(cells)[-1])
    assert key >> (27 + a) & 1 and key < 2 ** 30 and key >> 27 == 1 << a                                  # bit 27, 28 or 29 alone of the top three
    assert bc.single_grid(q)[0] == bc.AXIS


# ------------------------------------------------------------------------------------------------- 2. the cell limit
def test_cell_limit_fixtures():
    p, q = bc.cells_at_limit().points, bc.cells_over().points
    why, dims, ncell = bc.single_grid(p)
    assert why == bc.OK and dims == (1023, 512, 512) == ac.grid_of(p, 1.0)[2] and ncell == 268_173_312 <= 2 ** 28
    ids, n = bc.cell_ids(p)
    assert n == ncell and ids.max() == 268_173_311 and ids.min() == 0
    corner = np.array([(np.array(dims) - 1) * [(k >> i) & 1 for i in range(3)] for k in range(8)])
    cid = (corner[:, 2] * dims[1] + corner[:, 1]) * dims[0] + corner[:, 0]
    assert all((ids == c).sum() >= 10 for c in cid)                                   # a cluster in each of the eight corner cells
    i, j = ac.radius_pairs(p, 1.0)
    assert np.bincount(i, minlength=p.shape[0])[ids == ids.max()].min() >= 10         # the far corner's rows have neighbours to find
    why, dims, ncell = bc.single_grid(q)
    assert why == bc.CELLS and dims == (1023, 513, 512) == ac.grid_of(q, 1.0)[2] and ncell == 268_697_088 > 2 ** 28


# ------------------------------------------------------------------------------------------------- 3. chunk counts
def test_the_cut_cloud():
    ch = bc.cut_chunks()
    sizes = np.array([c.n for c in ch])
    assert len(ch) == 257 and sizes.min() == 1 and 35 <= sizes.max() <= 40
    for a, b in bc.ONE_ROW_RUNS:
        assert (sizes[a:b] == 1).all() and b - a >= 3
    assert ch[0].tarl.shape[1] == 16 and ch[0].dino.shape[1] == 32
    # all chunks lie in each other's space: most stored pairs of the whole cloud join rows of different chunks
    p = np.concatenate([c.points for c in ch])
    owner = np.repeat(np.arange(257), sizes)
    i, j = ac.radius_pairs(p, 1.0)
    assert (owner[i] != owner[j]).sum() > 20 * p.shape[0]


@pytest.mark.parametrize("nc", bc.CHUNK_COUNTS)
def test_chunk_counts_cross_their_thresholds(nc):
    c = bc.call(f"chunks_{nc}")
    assert len(c.chunks) == nc and c.plan().key() == (((0, nc),), ((0, nc),), (), None) and c.plan().blocks[(0, nc)] == 1
    clouds = [ch.points for ch in c.chunks]
    assert bc.order_keeps_chunks(bc.group_order(clouds), clouds)
    if nc in (17, 257):
        assert c.chunks[0] is bc.line_chunk("x") and c.chunks[-1] is bc.line_chunk("z")
        top = int(ac.morton_keys(ac.grid_of(clouds[-1], 1.0)[3]).max())
        assert top >> 29 == 1 and (nc - 1) == 1 << (bc.bits_for(nc) - 1)             # key bits 29 .. 30 + bits - 1 all matter: 1 0..0 | 1 ..
    assert [bc.bits_for(k) for k in (16, 17)] == [4, 5] and [bc.bits_for(k) for k in (255, 256, 257)] == [8, 8, 9]
    blocks_of_chunk_entries = -(-(nc + 1) // bc.AI_BLOCK)
    assert blocks_of_chunk_entries == (2 if nc >= 256 else 1)


# ------------------------------------------------------------------------------------------------- 4. plans
@pytest.mark.parametrize("name", sorted(bc.calls()))
def test_the_plan_is_the_claimed_one(name):
    c = bc.call(name)
    P = c.plan()
    assert P.built == c.built and P.split == c.split and P.error == c.error, (P.built, P.split, P.error)
    if c.blocks is not None:
        assert P.blocks[P.groups[0]] == c.blocks
    assert all(ch.n >= 1 for ch in c.chunks)
    if any(x in name for x in ("split", "cells")):
        assert c.big


def test_split_fixtures_sit_on_the_cell_limit():
    P = bc.call("split_pair").plan()
    assert P.cells[(0, 2)] == 2 ** 28 + 2 ** 18 and P.cells[(0, 1)] == 2 ** 27 + 2 ** 18 and P.cells[(1, 2)] == 2 ** 27
    assert bc.call("split_control").plan().cells == {(0, 2): 2 ** 28}
    P = bc.call("split_three").plan()
    assert P.cells[(0, 3)] > 2 ** 28 >= P.cells[(1, 3)] and len({c.n for c in bc.call("split_three").chunks}) == 1
    P = bc.call("split_deep").plan()
    assert P.cells[(0, 4)] == 2 ** 28 and P.cells[(4, 8)] == 4 * 87_994_368 > 2 ** 28 >= 3 * 87_994_368
    assert P.cells[(4, 6)] == P.cells[(6, 8)] == 2 * 87_994_368
    c = bc.call("split_second_group")
    assert c.group_rows == sum(ch.n for ch in c.chunks[:15]) and c.plan().groups == [(0, 15), (15, 17)]
    c = bc.call("split_then_error")
    assert c.plan().groups == [(0, 2), (2, 3)] and np.isnan(c.chunks[2].points).sum() == 1
    for name in ("split_pair", "split_three"):
        assert bc.call(name).theta and bc.call(name).gamma and bc.call(name).widest == 32


# ------------------------------------------------------------------------------------------------- 5. bounds
def _owner(n, S):
    """(block, thread, trip, trips of that thread) of every local row, by running the kernel's loop."""
    own = np.full((n, 4), -1)
    for s in range(S):
        for t in range(bc.AI_BLOCK):
            rows = bc.bounds_rows(n, S, s, t)
            for k, i in enumerate(rows):
                assert own[i, 0] == -1
                own[i] = (s, t, k, len(rows))
    assert (own[:, 0] >= 0).all()
    return own


@pytest.mark.parametrize("n,S,rows", [(4096, 1, (3840, 4095)), (4097, 2, (3840, 4095)), (8193, 3, (8192, 7679))])
def test_extreme_rows_belong_to_the_last_block_on_its_last_trip(n, S, rows):
    assert bc.bounds_blocks(n) == S and bc.extreme_rows(n) == rows
    own = _owner(n, S)
    r_min, r_max = rows
    assert own[r_min, :2].tolist() == [S - 1, 0] and own[r_max, :2].tolist() == [S - 1, 255]
    for r in rows:
        assert own[r, 2] == own[r, 3] - 1 >= 1                                          # the thread's last trip, and not its first
    c = bc.call(f"bounds_{n}")
    assert [ch.n for ch in c.chunks] == [1, n, 300]
    p = c.chunks[1].points
    assert p[r_min, 0] == 0.0 < np.delete(p[:, 0], r_min).min() and p[r_max, 0] == bc.axis_limit(0.0) > np.delete(p[:, 0], r_max).max() + 1.0
    assert bc.single_grid(p)[1] == (1023, 1, 1)
    for v, col, row in (("over", 0, r_max), ("nan", 1, r_max), ("+inf", 0, r_max), ("-inf", 2, r_min)):
        q = bc.call(f"bounds_{n}_{v}").chunks[1].points
        diff = np.argwhere(~((p == q) | (np.isnan(p) & np.isnan(q))))
        assert diff.tolist() == [[row, col]]                                            # the variants differ in that one coordinate
    assert bc.call(f"bounds_{n}_over").chunks[1].points[r_max, 0] == np.nextafter(bc.axis_limit(0.0), np.inf)


def test_bounds_cap():
    c = bc.call("bounds_cap")
    n = c.chunks[1].n
    assert n == 102 * 101 * 102 == 1_050_804 > 255 * 4096 and bc.bounds_blocks(n) == 256 == c.plan().blocks[(0, 2)]
    trips = [len(bc.bounds_rows(n, 256, s, t)) for s in (0, 255) for t in (0, 255)]
    assert max(trips) == 17 and min(trips) == 16
    p = c.chunks[1].points
    assert np.array_equal(p[0], p.min(0)) and np.array_equal(p[-1], p.max(0)) and bc.bounds_rows(n, 256, 8, 179)[-1] == n - 1
    assert sum(ch.n for ch in c.chunks) <= bc.DEFAULT_GROUP_ROWS


# ------------------------------------------------------------------------------------------------- 6. the chunk cap
def test_65536_chunks_are_groups_of_65535_and_1():
    p, off = bc.many_chunks()
    P = bc.group_plan(off, p)
    assert P.groups == [(0, 65535), (65535, 65536)] == P.built and not P.split and P.error is None
    assert bc.group_plan(off, p, chunk_cap=None).groups == [(0, 65536)]                 # what the parent's grouping gave: gridDim.y = 65536
    for at in (0, 65534):
        q, _ = bc.many_chunks(nan_at=at)
        P = bc.group_plan(off, q)
        assert P.error == (at, bc.NOT_FINITE) and P.built == [] and list(P.blocks) == [(0, 65535)]
    q, _ = bc.many_chunks(nan_at=65535)
    assert bc.group_plan(off, q).built == [(0, 65535)]


# ------------------------------------------------------------------------------------------------- the wrong models
ACCEPTED_BY = {
    "key_bits_short": ("chunks_1", "chunks_16", "chunks_255", "chunks_256"),
    "split_ge": ("split_pair", "split_three", "split_five"),
    "mid_up": ("split_pair", "split_control", "split_deep"),
    "first_trip_only": ("chunks_16", "split_pair"),
    "no_chunk_cap": ("chunks_257",),
}


def test_every_wrong_model_is_rejected_by_its_fixtures():
    table = {v: [n for n, c in bc.calls().items() if bc.rejects(c, v)] for v in bc.VARIANTS}
    p, off = bc.many_chunks()
    if bc.group_plan(off, p, chunk_cap=None).key() != bc.group_plan(off, p).key():
        table["no_chunk_cap"].append("many_chunks")
    for v in bc.VARIANTS:
        print(f"{v:16s} ({bc.VARIANTS[v]}) rejected by {', '.join(table[v])}")
    assert set(bc.REJECTED_BY) == set(bc.VARIANTS) == set(ACCEPTED_BY)
    for v in bc.VARIANTS:
        assert table[v], f"{v} is accepted everywhere"
        assert set(bc.REJECTED_BY[v]) <= set(table[v]), (v, sorted(set(bc.REJECTED_BY[v]) - set(table[v])))
        assert not set(ACCEPTED_BY[v]) & set(table[v]), (v, sorted(set(ACCEPTED_BY[v]) & set(table[v])))
