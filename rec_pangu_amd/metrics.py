"""Epoch metrics of device-resident predictions: binary ROC-AUC and log-loss without the host round trip.

`model_pipeline` ends every epoch with sklearn's `roc_auc_score` and `log_loss` over all predictions of the epoch: a copy of
every prediction to the host, an argsort and float64 cumulative sums on one thread.  For tensors on the HIP device the same two
numbers come from csrc/metrics.hip instead (rp_binary_metrics: key pass, the library's radix sort, a rank pass) as exact
integers (2U, P, N) and a float64 sum, read back in ONE 40-byte copy — the call's only synchronisation:

    roc_auc_score = 2U / (2 P N)        (ties counted as halves; one correctly rounded division of exact integers)
    log_loss      = logloss_sum / n     (q = clip(float64(p), 1e-7, 1 - 1e-7), the clipping model_pipeline.log_loss applies)

Everything the kernels do not define is left to the host path on the same data, so that the caller sees what sklearn returns
or raises today: CPU tensors, a non-finite prediction or a label that is neither 0 nor 1 (`unsupported` > 0), labels of one
class only (P == 0 or N == 0) and n >= 2^31 - 1.  The dispatch is by the tensors' device; there is no switch.
"""
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import hip

SUPPORTED_METRICS = ('roc_auc_score', 'log_loss')
EPS = 1e-7
MAX_N = 2 ** 31 - 1  # the sort's positions are int32


def _on_device(labels, preds) -> bool:
    return (isinstance(labels, torch.Tensor) and isinstance(preds, torch.Tensor) and labels.is_cuda and preds.is_cuda
            and 0 < preds.numel() < MAX_N and labels.numel() == preds.numel())


def _as_numpy(x) -> np.ndarray:
    return x.detach().reshape(-1).cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x).reshape(-1)


def _host_metrics(labels, preds, metric_list) -> Dict[str, float]:
    """today's path, unrounded: the functions are looked up in model_pipeline at call time (its clipping wrapper, and
    whatever a caller or a test put in place of sklearn's functions there)"""
    from . import model_pipeline as mp
    y, p = _as_numpy(labels), _as_numpy(preds)
    return {m: mp.log_loss(y, p, eps=EPS) if m == 'log_loss' else mp.roc_auc_score(y, p) for m in metric_list}


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().reshape(-1)
    return (t if t.dtype == torch.float32 else t.to(torch.float32)).contiguous()  # (a cast runs on the device)


def binary_counts(labels: torch.Tensor, preds: torch.Tensor, metric_list: Sequence[str] = SUPPORTED_METRICS) -> dict:
    """What the device returns for [n] device tensors: {'two_u', 'P', 'N', 'unsupported': ints, 'logloss_sum': float, 'n'}.
    two_u is 0 when 'roc_auc_score' is not asked for and logloss_sum 0.0 when 'log_loss' is not."""
    if not _on_device(labels, preds):
        raise RuntimeError("binary_counts: needs two HIP-device tensors of one length n, 0 < n < 2^31 - 1")
    flags = (hip.METRIC_AUC if 'roc_auc_score' in metric_list else 0) | (hip.METRIC_LOGLOSS if 'log_loss' in metric_list else 0)
    res = hip.binary_metrics(_f32(preds), _f32(labels), flags, EPS)
    host = res.cpu().numpy()  # the one device-to-host copy (and the one wait)
    return {"two_u": int(host[0]), "P": int(host[1]), "N": int(host[2]), "unsupported": int(host[3]),
            "logloss_sum": float(host[4:5].view(np.float64)[0]), "n": int(preds.numel())}


def auc_counts(labels: torch.Tensor, preds: torch.Tensor) -> Tuple[int, int, int]:
    """(2U, P, N) of device tensors, exact: roc_auc_score = 2U / (2 P N)"""
    c = binary_counts(labels, preds, ('roc_auc_score',))
    return c["two_u"], c["P"], c["N"]


def binary_metrics(labels, preds, metric_list: Sequence[str]) -> Dict[str, float]:
    """{metric: unrounded float64} for the metrics named ('roc_auc_score', 'log_loss'), of all predictions of an epoch."""
    for m in metric_list:
        assert m in SUPPORTED_METRICS, 'metric :{} not supported! metric must be in {}'.format(m, list(SUPPORTED_METRICS))
    if not metric_list:
        return {}
    if not _on_device(labels, preds):
        return _host_metrics(labels, preds, metric_list)
    c = binary_counts(labels, preds, metric_list)
    if c["unsupported"] > 0 or c["P"] == 0 or c["N"] == 0:
        return _host_metrics(labels, preds, metric_list)
    out = {}
    for m in metric_list:
        if m == 'log_loss':
            out[m] = np.float64(c["logloss_sum"] / c["n"])
        else:
            out[m] = np.float64(c["two_u"] / (2 * c["P"] * c["N"]))  # int / int: correctly rounded, also beyond 2^53
    return out
