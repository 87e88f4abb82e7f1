"""Host side of the device epoch metrics (rec_pangu_amd/metrics.py, csrc/metrics.hip): the exact integer formulation of
ROC-AUC restated in numpy and held against sklearn, the C entry points' argument checks (no GPU needed), and the host path
of `metrics.binary_metrics` — for CPU tensors it is `model_pipeline._metric` before rounding, whatever that returns or raises.

    AUC = 2U / (2 P N),  2U = sum over positives of (#negatives with a smaller prediction + #negatives with one <= it)
"""
import ctypes
import warnings

import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score


def float_keys(p):
    """the order-preserving int32 key of float32 predictions: both zeros are one key, signed integer order == float order"""
    f = np.asarray(p, dtype=np.float32) + np.float32(0.0)  # -0.0 + 0.0 = +0.0
    k = f.view(np.int32).copy()
    k[k < 0] ^= np.int32(0x7FFFFFFF)
    return k


def exact_counts(y, p):
    """(2U, P, N) as Python ints: stable argsort of the keys, cumulative negative counts, tie groups by their boundaries"""
    y = np.asarray(y)
    k = float_keys(p)
    order = np.argsort(k, kind="stable")
    ks, ys = k[order], y[order]
    neg, pos = (ys == 0).astype(np.int64), ys == 1
    start = np.ones(len(ks), dtype=bool)
    start[1:] = ks[1:] != ks[:-1]
    gid = np.cumsum(start) - 1                      # tie group of every sorted element
    before = np.cumsum(neg) - neg                   # negatives at sorted places before it
    nc = np.concatenate([before[start], [neg.sum()]])  # negatives before group g; one past the last group: all of them
    two_u = int((nc[gid[pos]] + nc[gid[pos] + 1]).sum())
    return two_u, int(pos.sum()), int(neg.sum())


def exact_auc(y, p):
    two_u, P, N = exact_counts(y, p)
    return two_u / (2 * P * N)


def labelled(n, seed, kind):
    rng = np.random.default_rng(seed)
    p = rng.random(n).astype(np.float32)
    if kind == "quantised":
        p = (rng.integers(0, 4, n) / 4).astype(np.float32)
    y = (rng.random(n) < 0.5).astype(np.float32)
    y[0], y[1] = 1.0, 0.0
    return y, p


@pytest.mark.parametrize("kind", ["continuous", "quantised"])
@pytest.mark.parametrize("n", [2, 17, 4097, 100001])
def test_integer_formulation_agrees_with_sklearn(n, kind):
    """within n * 2^-52: sklearn's trapezoid sum makes at most n roundings of terms <= 1; the rational is rounded once"""
    y, p = labelled(n, 7 + n, kind)
    got, want = exact_auc(y, p), roc_auc_score(y, p)
    print(f"n={n} {kind}: |exact - sklearn| = {abs(got - want):.3e}")
    assert abs(got - want) <= n * 2.0 ** -52


def test_integer_formulation_on_hand_checked_cases():
    assert exact_counts([1, 0], [0.0, -0.0]) == (1, 1, 1)             # the two zeros tie: AUC 0.5
    assert exact_counts([1, 0], [1e-40, 0.0]) == (2, 1, 1)            # a denormal is above zero
    assert exact_counts([0, 1, 0, 1], [-1.0, -0.5, 0.25, 0.25]) == (2 + 3, 2, 2)
    assert exact_counts([0, 1, 1, 0], [0.3] * 4) == (4, 2, 2)         # one group: exactly 0.5


def test_workspace_size_is_positive_and_grows():
    from rec_pangu_amd import hip
    lib = hip.lib()
    sizes = []
    for n in (1, 4096, 4097, 100001, 45_000_000):
        b = ctypes.c_size_t(0)
        assert lib.rp_metrics_workspace_bytes(n, ctypes.byref(b)) == 0
        sizes.append(b.value)
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[-1] < 24 * 45_000_000  # ~21 bytes per element


def test_argument_validation_needs_no_gpu():
    """every refusal happens before anything touches the device: -1 and a message, with host memory standing in for buffers"""
    from rec_pangu_amd import hip
    lib = hip.lib()
    b = ctypes.c_size_t(0)
    assert lib.rp_metrics_workspace_bytes(8, None) == -1 and b"null" in lib.rp_last_error()
    for bad in (0, -3, 2 ** 31 - 1, 2 ** 40):
        assert lib.rp_metrics_workspace_bytes(bad, ctypes.byref(b)) == -1 and b"outside" in lib.rp_last_error()
    n = 100
    assert lib.rp_metrics_workspace_bytes(n, ctypes.byref(b)) == 0
    ws = ctypes.create_string_buffer(b.value)
    pred, label = (ctypes.c_float * n)(), (ctypes.c_float * n)()
    res = (ctypes.c_int64 * 5)()
    a = ctypes.addressof

    def call(ws_p=a(ws), ws_n=b.value, p=a(pred), y=a(label), n_=n, eps=1e-7, flags=3, r=a(res)):
        return lib.rp_binary_metrics(ws_p, ws_n, p, y, n_, eps, flags, r, None)

    for kw in (dict(ws_p=None), dict(p=None), dict(y=None), dict(r=None)):
        assert call(**kw) == -1 and b"null" in lib.rp_last_error()
    for bad in (0, -1, 2 ** 31 - 1):
        assert call(n_=bad) == -1 and b"outside" in lib.rp_last_error()
    assert call(ws_n=b.value - 1) == -1 and b"workspace" in lib.rp_last_error()
    assert call(flags=0) == -1 and call(flags=4) == -1 and b"flags" in lib.rp_last_error()
    assert call(y=a(pred)) == -1 and b"alias" in lib.rp_last_error()
    assert call(y=a(pred) + 4 * (n - 1)) == -1 and b"alias" in lib.rp_last_error()  # partial overlap
    assert call(r=a(label) + 8) == -1 and b"alias" in lib.rp_last_error()
    assert call(p=a(ws) + 512) == -1 and b"alias" in lib.rp_last_error()
    assert call(r=a(ws) + 64) == -1 and b"alias" in lib.rp_last_error()


def _outcome(f):
    """('value', x) or ('raised', exception type) with warnings kept quiet; nan == nan"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            v = f()
        except Exception as e:  # noqa: BLE001 - the type is what is compared
            return ("raised", type(e))
    return ("value", "nan" if np.isnan(v) else float(v))


def test_cpu_tensors_take_the_host_path_unrounded():
    from rec_pangu_amd import metrics
    from rec_pangu_amd import model_pipeline as mp
    for n, kind in ((50, "continuous"), (4097, "quantised"), (1000, "continuous")):
        y, p = labelled(n, 3 + n, kind)
        got = metrics.binary_metrics(torch.from_numpy(y), torch.from_numpy(p), ["roc_auc_score", "log_loss"])
        assert list(got) == ["roc_auc_score", "log_loss"]
        assert got["roc_auc_score"] == roc_auc_score(y, p) and got["log_loss"] == mp.log_loss(y, p, eps=1e-7)
        for m in got:
            assert round(got[m], 4) == mp._metric(m, y, p)
        assert list(metrics.binary_metrics(torch.from_numpy(y), torch.from_numpy(p), ["log_loss"])) == ["log_loss"]
    assert metrics.binary_metrics(torch.zeros(3), torch.zeros(3), []) == {}
    with pytest.raises(AssertionError, match="not supported"):
        metrics.binary_metrics(torch.zeros(3), torch.zeros(3), ["accuracy"])
    with pytest.raises(RuntimeError, match="HIP-device"):
        metrics.auc_counts(torch.zeros(3), torch.zeros(3))


@pytest.mark.parametrize("case", ["all_positive", "all_negative", "nan_prediction", "half_label"])
@pytest.mark.parametrize("metric", ["roc_auc_score", "log_loss"])
def test_undefined_inputs_do_what_the_pipeline_does_today(case, metric):
    from rec_pangu_amd import metrics
    from rec_pangu_amd import model_pipeline as mp
    y, p = labelled(64, 11, "continuous")
    if case == "all_positive":
        y[:] = 1.0
    elif case == "all_negative":
        y[:] = 0.0
    elif case == "nan_prediction":
        p[5] = np.nan
    else:
        y[7] = 0.5
    want = _outcome(lambda: mp._metric(metric, y, p))
    got = _outcome(lambda: round(metrics.binary_metrics(torch.from_numpy(y), torch.from_numpy(p), [metric])[metric], 4))
    assert got == want, (case, metric, got, want)


def test_cpu_trainer_loop_is_unchanged(monkeypatch):
    """host chunks never reach rec_pangu_amd.metrics: model_pipeline._epoch_metrics is _to_host + _metric for them"""
    from rec_pangu_amd import metrics
    from rec_pangu_amd import model_pipeline as mp
    monkeypatch.setattr(metrics, "binary_metrics", lambda *a, **k: pytest.fail("host chunks went to the device module"))
    y, p = labelled(300, 5, "continuous")
    yc, pc = [torch.from_numpy(c) for c in np.split(y, 3)], [torch.from_numpy(c).reshape(-1, 1) for c in np.split(p, 3)]
    got = mp._epoch_metrics(yc, pc, ["roc_auc_score", "log_loss"])
    assert got == {m: mp._metric(m, y, p) for m in ("roc_auc_score", "log_loss")}
