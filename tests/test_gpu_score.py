"""GPU: the scorer's tail on resident labels -- `remove_semantics`, `score_sweep`, `Metrics.update_stats` on tensors -- against
``oracle/metrics_ref.score`` and the NumPy restatement of tests/score_ref.py, exactly."""
import os

import numpy as np
import pytest

import score_ref as sr
from conftest import GOLDEN
from oracle import metrics_ref

pytestmark = pytest.mark.gpu


def same(got, exp, what):
    assert set(exp) <= set(got), what
    for key, v in exp.items():
        assert got[key] == v or (isinstance(v, float) and np.isnan(v) and np.isnan(got[key])), (what, key, got[key], v)


@pytest.fixture(scope="module")
def stacked():
    """scorer_a / scorer_b, each stacked with two permuted copies of itself (a relabelling that keeps 0) and one row whose instances
    lie on the ground: {name: (preds (4, n), gt)}."""
    out = {}
    for name in ("scorer_a", "scorer_b"):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        pred, gt = z["pred"].astype(np.int32), z["gt"].astype(np.int32)
        rng = np.random.default_rng(len(name) + pred.size)
        rows = [pred]
        top = int(pred.max()) + 1
        for _ in range(2):
            m = np.concatenate([[0], 1 + rng.permutation(top + 5)])[: top + 1]
            rows.append(np.where(pred >= 0, m[np.maximum(pred, 0)], pred).astype(np.int32))
        ground = np.where((gt == 0) & (rng.random(gt.size) < 0.9), top + 7 + (np.arange(gt.size) % 3), pred).astype(np.int32)
        rows.append(ground)
        out[name] = (np.stack(rows), gt)
    return out


@pytest.mark.parametrize("name", ["scorer_a", "scorer_b"])
@pytest.mark.parametrize("device", [False, True])
def test_score_sweep_without_removal(ctx, stacked, name, device):
    from autoinst_amd import labels_api
    preds, gt = stacked[name]
    p, g = preds, gt
    if device:
        import torch
        p, g = torch.as_tensor(preds, device="cuda"), torch.as_tensor(gt, device="cuda")
    got = labels_api.score_sweep(p, g, 200, remove=False, ctx=ctx)
    assert len(got) == preds.shape[0]
    for t in range(preds.shape[0]):
        same(got[t], metrics_ref.score(preds[t], preds[t], gt, 200), (name, t))


@pytest.mark.parametrize("name", ["scorer_a", "scorer_b"])
def test_score_sweep_with_removal(ctx, stacked, name):
    import torch
    from autoinst_amd import labels_api
    preds, gt = stacked[name]
    got = labels_api.score_sweep(torch.as_tensor(preds, device="cuda"), torch.as_tensor(gt, device="cuda"), 200, remove=True, ctx=ctx)
    changed = 0
    for t in range(preds.shape[0]):
        removed = sr.remove_semantics(gt, preds[t], 0.8)
        changed += int((removed != preds[t]).sum())
        same(got[t], metrics_ref.score(preds[t], removed, gt, 200), (name, t))
    assert changed > 0


@pytest.mark.parametrize("name", ["scorer_a", "scorer_b"])
def test_remove_semantics_is_the_drop_in(ctx, stacked, name):
    import torch
    from autoinst_amd import labels_api
    preds, gt = stacked[name]
    for t in (0, 3):
        exp = sr.remove_semantics(gt, preds[t].astype(np.int64), 0.8)
        got = labels_api.remove_semantics(gt, preds[t].astype(np.int64), 0.8, num_threads=4, ctx=ctx)
        assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, exp)
        dev = labels_api.remove_semantics(torch.as_tensor(gt, device="cuda"), torch.as_tensor(preds[t], device="cuda"), ctx=ctx)
        assert dev.is_cuda and dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), exp)
    assert np.array_equal(labels_api.remove_semantics(gt, preds[3], 0.0, ctx=ctx), sr.remove_semantics(gt, preds[3], 0.0))


def test_metrics_update_stats_on_tensors_equals_host_copies(ctx, stacked):
    import torch
    from autoinst_amd import labels_api
    preds, gt = stacked["scorer_a"]
    removed = sr.remove_semantics(gt, preds[3], 0.8)
    host, dev = labels_api.Metrics("h", min_points=200, ctx=ctx), labels_api.Metrics("d", min_points=200, ctx=ctx)
    for alll, pred in ((preds[3], removed), (preds[1], preds[1])):
        a = host.update_stats(alll, pred, gt)
        ta, tp = torch.as_tensor(alll, device="cuda"), torch.as_tensor(pred, device="cuda")
        b = dev.update_stats(ta, tp if pred is not alll else ta, torch.as_tensor(gt, device="cuda"))
        assert a == b
    assert host.sequence_metrics == dev.sequence_metrics


def test_score_sweep_of_a_cut_tree_left_on_the_device(ctx):
    """ncuts_tree + relabel of one 20k chunk at 4 thresholds, the labels never leaving the device."""
    import torch
    from autoinst_amd import labels_api, ncuts_api, synth
    ch = synth.synthetic_chunk(20_000, 11, tarl=True)
    g = ncuts_api.build_affinity(ch["points"], ch["tarl"], alpha=1.0, theta=0.5, gamma=0.0, ctx=ctx)
    tree = ncuts_api.ncuts_tree(g, 20_000, 0.03)
    g.free()
    labels, _ = ncuts_api.relabel([tree], [0.005, 0.01, 0.02, 0.03], device=torch.device("cuda"), ctx=ctx)
    gt = ch["gt"].copy()
    gt[::97] = 0
    rows = [labels[t][0] + 1 for t in range(4)]
    assert all(r.is_cuda for r in rows)
    tg = torch.as_tensor(gt, device="cuda")
    for remove in (False, True):
        got = labels_api.score_sweep(rows, tg, 200, remove=remove, ctx=ctx)
        for t in range(4):
            p = rows[t].cpu().numpy()
            same(got[t], metrics_ref.score(p, sr.remove_semantics(gt, p, 0.8) if remove else p, gt, 200), (remove, t))
    # relabel's own buffers (a list of per-chunk views per threshold) are taken as they are
    raw = labels_api.label_tables(labels, tg, min_points=200, ctx=ctx)
    assert len(raw) == 4 and all(int(t[2].sum()) == 20_000 for t in raw)
