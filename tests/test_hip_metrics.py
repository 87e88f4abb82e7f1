"""Epoch metrics on the device (csrc/metrics.hip through rec_pangu_amd/metrics.py): (2U, P, N) equal the numpy restatement of
test_metrics_host.py as INTEGERS at the tile edges (a wave round is 64 elements, a tile 4096), with tie groups inside a round,
across tiles and over the whole array; the float64 log-loss sum against model_pipeline.log_loss; bit-identical repeats; the
host path for what the kernels do not define; and the trainers' dicts with sklearn taken away."""
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import log_loss as sk_log_loss
from sklearn.metrics import roc_auc_score as sk_roc_auc_score

from conftest import require_gpu, small_enc_dict
from test_metrics_host import _outcome, exact_counts

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [2, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 1, 100001]
BOTH = ["roc_auc_score", "log_loss"]
SPECIALS = np.array([0.0, -0.0, 1.0, 1e-40, -0.25, -1e-40, -3.5, 0.0, -0.0, 1.0], dtype=np.float32)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    require_gpu()
    from rec_pangu_amd import hip
    hip.lib()


def _labels(rng, n):
    y = (rng.random(n) < 0.5).astype(np.float32)
    y[0], y[1] = 1.0, 0.0
    return y


def _preds(kind, n, rng):
    if kind == "distinct":
        return ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    if kind == "four_levels":  # 0.0, 0.25, 0.5, 0.75: tie groups of ~n/4 elements, across tiles from n = 4097 on
        return (rng.integers(0, 4, n) / 4).astype(np.float32)
    if kind == "all_equal":
        return np.full(n, 0.3, dtype=np.float32)
    assert kind == "specials"  # both zeros (one tie group), 1.0, denormals of both signs, negative values
    p = (rng.random(n) * 2 - 1).astype(np.float32)
    p[:min(n, len(SPECIALS))] = SPECIALS[:n]
    return p


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.mark.parametrize("n", SIZES)
def test_auc_counts_are_the_exact_integers(n):
    from rec_pangu_amd import metrics
    rng = np.random.default_rng(100 + n)
    for kind in ("distinct", "four_levels", "all_equal", "specials"):
        y, p = _labels(rng, n), _preds(kind, n, rng)
        if kind == "distinct":
            assert len(np.unique(p)) == n
        want = exact_counts(y, p)
        got = metrics.auc_counts(_dev(y), _dev(p))
        assert got == want, (n, kind, got, want)
        assert all(isinstance(v, int) for v in got)
        if kind == "all_equal":
            assert got[0] == got[1] * got[2]  # AUC exactly 0.5
            assert metrics.binary_metrics(_dev(y), _dev(p), ["roc_auc_score"])["roc_auc_score"] == 0.5
        if n == 100001 and kind == "distinct":
            # half positives: 2U = 2 AUC P N.  Unrelated predictions (AUC ~ 0.5) pass 2^31; predictions that rank every
            # positive above every negative give 2U = 2 P N ~ 5e9 and pass 2^32: no 32-bit accumulator holds either
            assert got[0] > 2 ** 31
            ranked = np.where(y == 1, p + 1, p).astype(np.float32)
            want = exact_counts(y, ranked)
            assert want[0] == 2 * want[1] * want[2] > 2 ** 32
            assert metrics.auc_counts(_dev(y), _dev(ranked)) == want
            assert metrics.binary_metrics(_dev(y), _dev(ranked), ["roc_auc_score"])["roc_auc_score"] == 1.0


@pytest.mark.parametrize("n", SIZES)
def test_one_positive_at_the_smallest_the_largest_and_inside_a_tie_group_across_a_tile_edge(n):
    from rec_pangu_amd import metrics
    rng = np.random.default_rng(200 + n)
    p = ((rng.permutation(n) + 0.5) / n).astype(np.float32)
    for where in (int(np.argmin(p)), int(np.argmax(p))):
        y = np.zeros(n, dtype=np.float32)
        y[where] = 1.0
        want = (0 if where == int(np.argmin(p)) else 2 * (n - 1), 1, n - 1)
        assert exact_counts(y, p) == want
        assert metrics.auc_counts(_dev(y), _dev(p)) == want, (n, where)
    if n > 4096:
        # sorted places 4000 .. min(n, 4200) - 1 share one value: the group straddles elements 4095 / 4096 of the sorted order
        lo, hi = 4000, min(n, 4200)
        order = np.argsort(p, kind="stable")
        p[order[lo:hi]] = p[order[lo]]
        for member in (lo, 4095, 4096, hi - 1):
            y = np.zeros(n, dtype=np.float32)
            y[order[member]] = 1.0
            want = (lo + (lo + (hi - lo - 1)), 1, n - 1)  # negatives below the group + those up to its end
            assert exact_counts(y, p) == want
            assert metrics.auc_counts(_dev(y), _dev(p)) == want, (n, member)


def test_log_loss_sum_against_the_pipelines_log_loss():
    """relative max(1e-13, n 2^-52): a float64 sum in another order plus a few ulp of the device's log"""
    from rec_pangu_amd import metrics
    from rec_pangu_amd import model_pipeline as mp
    worst = 0.0
    for n in SIZES:
        rng = np.random.default_rng(300 + n)
        for kind in ("distinct", "four_levels", "specials"):
            y, p = _labels(rng, n), _preds(kind, n, rng)
            want = mp.log_loss(y, p, eps=1e-7)
            c = metrics.binary_counts(_dev(y), _dev(p), ["log_loss"])
            assert c["n"] == n and c["two_u"] == 0 and c["unsupported"] == 0
            got = c["logloss_sum"] / n
            rel = abs(got - want) / abs(want)
            worst = max(worst, rel)
            assert np.isfinite(got) and rel <= max(1e-13, n * 2.0 ** -52), (n, kind, got, want, rel)
            assert metrics.binary_metrics(_dev(y), _dev(p), ["log_loss"])["log_loss"] == got
    print(f"largest relative difference of the device log-loss: {worst:.3e}")
    # predictions 0.0 and 1.0: the clipped values, not inf.  On the wrong side that is -log(q) at q = 1e-7 for the positive
    # and -log(1 - q) at q = 1 - 1e-7 for the negative (in float64 1 - (1 - 1e-7) is 1e-7 (1 + 5.8e-9): what the host computes too)
    hi = 1.0 - 1e-7
    for y2, want in (([1, 0], -(np.log(1e-7) + np.log(1.0 - hi)) / 2), ([0, 1], -(np.log(1.0 - 1e-7) + np.log(hi)) / 2)):
        y2, p2 = np.array(y2, np.float32), np.array([0.0, 1.0], np.float32)
        got = metrics.binary_counts(_dev(y2), _dev(p2), ["log_loss"])["logloss_sum"] / 2
        assert np.isfinite(got) and abs(got - want) <= 1e-13 * abs(want), (y2, got, want)
        assert abs(got - mp.log_loss(y2, p2, eps=1e-7)) <= 1e-13 * abs(want)
    assert abs(want - 1e-7) < 1e-13 and abs(metrics.binary_counts(_dev(np.array([1, 0], np.float32)), _dev(p2), ["log_loss"])
                                            ["logloss_sum"] / 2 + np.log(1e-7)) < 1e-9 * 16.2


def test_repeats_are_bit_identical_and_independent_of_what_lies_behind_n():
    from rec_pangu_amd import hip
    rng = np.random.default_rng(5)
    for n in (4097, 100001):
        y, p = _dev(_labels(rng, n)), _dev(_preds("four_levels" if n == 4097 else "distinct", n, rng))
        a, b = hip.binary_metrics(p, y).cpu(), hip.binary_metrics(p, y).cpu()
        assert torch.equal(a, b)
        long_p = torch.full((3 * n + 17,), float("nan"), device=DEV)
        long_y = torch.full((3 * n + 17,), 0.5, device=DEV)
        long_p[:n], long_y[:n] = p, y
        c = hip.binary_metrics(long_p[:n], long_y[:n]).cpu()
        assert torch.equal(a, c)
        assert int(a[3]) == 0 and int(a[1]) + int(a[2]) == n
    # the stages issued one call at a time over one workspace are the whole call
    ws, res = hip.metrics_workspace(n, y.device), torch.zeros(5, dtype=torch.int64, device=DEV)
    hip.binary_metrics(p, y, workspace=ws, result=res, stages=list(hip.METRICS_STAGES))
    assert torch.equal(res.cpu(), a)


def test_other_dtypes_are_cast_on_the_device():
    from rec_pangu_amd import metrics
    rng = np.random.default_rng(9)
    y, p = _labels(rng, 1000), _preds("four_levels", 1000, rng)
    want = exact_counts(y, p)
    assert metrics.auc_counts(_dev(y.astype(np.int64)), _dev(p.astype(np.float64))) == want
    assert metrics.auc_counts(_dev(y).reshape(-1, 1), _dev(p).reshape(-1, 1).to(torch.bfloat16)) == want  # (quarters are exact)


def test_unsupported_elements_are_counted_exactly_and_take_the_host_path():
    from rec_pangu_amd import metrics
    rng = np.random.default_rng(17)
    n = 5000
    y, p = _labels(rng, n), _preds("distinct", n, rng)
    p[[3, 4097, 4999]] = np.nan
    p[[64, 65]] = [np.inf, -np.inf]
    y[[10, 4096, 4097, 200]] = [0.5, 2.0, -1.0, np.nan]  # element 4097 is bad twice and counts once
    assert metrics.binary_counts(_dev(y), _dev(p))["unsupported"] == 8
    y2, p2 = _labels(rng, n), _preds("distinct", n, rng)
    for case in ("nan_prediction", "half_label", "all_positive", "all_negative"):
        yy, pp = y2.copy(), p2.copy()
        if case == "nan_prediction":
            pp[77] = np.nan
        elif case == "half_label":
            yy[4100] = 0.5
        else:
            yy[:] = 1.0 if case == "all_positive" else 0.0
        for metric in BOTH:
            want = _outcome(lambda: metrics.binary_metrics(torch.from_numpy(yy), torch.from_numpy(pp), [metric])[metric])
            got = _outcome(lambda: metrics.binary_metrics(_dev(yy), _dev(pp), [metric])[metric])
            assert got == want, (case, metric, got, want)


# ---- the trainers ---------------------------------------------------------------------------------------------------------
class _Loader:
    """the little of a DataLoader that train_model / test_model use: dict batches of host tensors, fresh dicts every epoch"""

    def __init__(self, batches):
        self.batches, self.batch_size = batches, len(batches[0]["label"])
        self.dataset = range(sum(len(b["label"]) for b in batches))

    def __iter__(self):
        return iter([dict(b) for b in self.batches])


def _host_batches(enc, sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for B in sizes:
        b = {k: (torch.rand(B, generator=gen) if "min" in v else torch.randint(0, v["vocab_size"] + 1, (B,), generator=gen))
             for k, v in enc.items()}
        for name, rate in (("label", 0.3), ("task1_label", 0.3), ("task2_label", 0.15)):
            b[name] = (torch.rand(B, generator=gen) < rate).float()
        out.append(b)
    return out


def _no_sklearn(*a, **k):
    raise AssertionError("the trainer went to sklearn for device-resident predictions")


def _away_from_rounding_edges(values):
    return all(abs((v * 1e4) % 1.0 - 0.5) > 1e-5 for v in values)  # no value within 1e-9 of a 4-decimal rounding edge


def _run_and_compare(monkeypatch, run, prefix, num_task):
    """run() -> the trainer's dict with sklearn taken out of model_pipeline; the tensors it handed to the device metrics are
    copied to the host and give the expected dict through sklearn itself -> (equal?, no value near a rounding edge?)"""
    from rec_pangu_amd import metrics
    from rec_pangu_amd import model_pipeline as mp
    seen = []
    real = metrics.binary_metrics

    def spy(labels, preds, metric_list):
        assert labels.is_cuda and preds.is_cuda
        seen.append((labels.detach().cpu().numpy().copy(), preds.detach().cpu().numpy().copy()))
        return real(labels, preds, metric_list)

    with monkeypatch.context() as m:
        m.setattr(metrics, "binary_metrics", spy)
        m.setattr(mp, "roc_auc_score", _no_sklearn)
        m.setattr(mp, "_sk_log_loss", _no_sklearn)
        got = run()
    assert len(seen) == num_task
    want, raw = {}, []
    for i, (y, p) in enumerate(seen):
        vals = {"roc_auc_score": sk_roc_auc_score(y, p), "log_loss": sk_log_loss(y, np.clip(p.astype(np.float64), 1e-7, 1 - 1e-7))}
        raw += list(vals.values())
        for name, v in vals.items():
            want[f"{prefix}{name}" if num_task == 1 else f"{prefix}task{i + 1}_{name}"] = round(v, 4)
    if not _away_from_rounding_edges(raw):
        return None
    assert got == want, (got, want)
    return got


@pytest.mark.parametrize("mode", ["test_model", "train_eager", "train_graphed"])
@pytest.mark.parametrize("kind", ["deepfm", "mmoe"])
def test_trainers_return_the_sklearn_dicts_without_sklearn(kind, mode, monkeypatch):
    from rec_pangu_amd import model_pipeline as mp
    from rec_pangu_amd.graph_step import GraphedTrainStep
    from rec_pangu_amd.models.layers.embedding import EmbeddingLayer
    from rec_pangu_amd.optim import FusedAdam
    enc = small_enc_dict()
    num_task = 2 if kind == "mmoe" else 1
    dev = torch.device(DEV)
    try:
        for seed in (0, 1, 2, 3):  # the next seed only if a value of this one lies on a 4-decimal rounding edge
            torch.manual_seed(seed)
            if kind == "mmoe":
                from rec_pangu_amd.models.multi_task import MMOE
                model = MMOE(enc_dict=enc, embedding_dim=8, device=None).to(dev)
            else:
                from rec_pangu_amd.models.ranking import DeepFM
                model = DeepFM(embedding_dim=8, hidden_units=[16, 8], enc_dict=enc).to(dev)
            loader = _Loader(_host_batches(enc, [128] * 6 + [37], 40 + seed))
            if mode == "test_model":
                res = _run_and_compare(monkeypatch, lambda: mp.test_model(model, loader, dev, num_task=num_task),
                                       "" if num_task == 1 else "test_", num_task)
            else:
                for m in model.modules():
                    if hasattr(m, "check_indices"):
                        m.check_indices = "deferred"
                opt = FusedAdam(model.parameters(), lr=1e-2, fuse_zero_grad=True, lazy_tables=True, replay="closed")
                gstep = GraphedTrainStep(model, opt) if mode == "train_graphed" else None
                res = _run_and_compare(monkeypatch, lambda: mp.train_model(model, loader, opt, dev, num_task=num_task,
                                                                           graphed_step=gstep), "train_", num_task)
                if gstep is not None and res is not None:
                    assert gstep.replays >= 2
            if res is not None:
                break
        assert res is not None, "every seed put a value on a rounding edge"
        assert len(res) == 2 * num_task
        # one metric alone is computed alone
        one = mp.test_model(model, loader, dev, metric_list=["log_loss"], num_task=num_task)
        assert len(one) == num_task and all(k.endswith("log_loss") for k in one)
    finally:
        EmbeddingLayer.unpin_sorts()
