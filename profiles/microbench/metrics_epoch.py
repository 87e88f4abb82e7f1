"""The end of an epoch: ROC-AUC + log-loss over all predictions of the epoch, held on the HIP device as the trainers hold them
(one chunk per batch of 65 536).  Two ways to the same two numbers, on the same box and the same data:

  device  model_pipeline._epoch_metrics as it stands: the chunks joined on the device, rp_binary_metrics (key pass, radix sort,
          rank pass), ONE 40-byte copy back.  HIP events around `--calls` calls after `--warmup`, ending in a synchronise, and a
          host clock around the same calls.
  host    the parent's path: model_pipeline._to_host of both chunk lists (torch.cat + .cpu() + .numpy()) and
          model_pipeline._metric for both metrics (sklearn: argsort and float64 cumulative sums on one thread).  Host clock,
          median of `--host-repeats`.

Per-launch times come from a separate short run that issues the entry point's launches one call at a time under
hip.enable_timing (events around every call serialise them), with the algorithmic bytes of each and their share of 8 TB/s.

    python profiles/microbench/metrics_epoch.py [--sizes 65536 4194304 45000000] [--out FILE]

Prints one JSON line per n.  Needs an MI355X: there is no CPU timing path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rec_pangu_amd import hip, metrics  # noqa: E402
from rec_pangu_amd import model_pipeline as mp  # noqa: E402

DEV = "cuda"
BOTH = ["roc_auc_score", "log_loss"]
CHUNK = 65536
HBM_BYTES_PER_S = 8e12
BYTES_PER_ELEMENT = 40  # chunks + joined tensors (16) + the workspace (~21) + slack: what one size needs on the device


def make_chunks(n, seed):
    """predictions in (0, 1) and labels drawn with a probability that follows them (AUC ~ 0.7), in chunks of one batch"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    preds, labels = [], []
    for lo in range(0, n, CHUNK):
        m = min(CHUNK, n - lo)
        p = torch.rand(m, 1, device=DEV, generator=gen)
        y = (torch.rand(m, device=DEV, generator=gen) < 0.1 + 0.6 * p[:, 0]).float()
        preds.append(p)
        labels.append(y)
    return labels, preds


def host_path(labels, preds):
    y, p = mp._to_host(labels), mp._to_host(preds)
    return {m: mp._metric(m, y, p) for m in BOTH}


def run(n, warmup, calls, host_repeats):
    free, _ = torch.cuda.mem_get_info()
    if n * BYTES_PER_ELEMENT > free:
        print(f"n = {n}: skipped, needs ~{n * BYTES_PER_ELEMENT / 2 ** 30:.1f} GiB of device memory, {free / 2 ** 30:.1f} GiB free",
              flush=True)
        return None
    labels, preds = make_chunks(n, 1234)
    res = {"n": n, "chunks": len(preds), "warmup": warmup, "calls": calls, "host_repeats": host_repeats,
           "host_threads": {"torch": torch.get_num_threads(), "affinity": len(os.sched_getaffinity(0)),
                            "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS")}}

    for _ in range(warmup):
        dev_vals = mp._epoch_metrics(labels, preds, BOTH)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(calls):
        dev_vals = mp._epoch_metrics(labels, preds, BOTH)
    e1.record()
    torch.cuda.synchronize()
    res["device_ms_host_clock"] = (time.perf_counter() - t0) * 1e3 / calls
    res["device_ms_events"] = e0.elapsed_time(e1) / calls
    res["device_values"] = {k: float(v) for k, v in dev_vals.items()}

    times = []
    for _ in range(host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_vals = host_path(labels, preds)
        times.append((time.perf_counter() - t0) * 1e3)
    res["host_ms_host_clock"] = statistics.median(times)
    res["host_ms_all"] = times
    res["host_values"] = {k: float(v) for k, v in host_vals.items()}
    res["values_equal"] = res["host_values"] == res["device_values"]
    res["host_over_device"] = res["host_ms_host_clock"] / res["device_ms_host_clock"]

    # the launches one call at a time (a run of its own: the events serialise them)
    y, p = torch.cat([c.reshape(-1) for c in labels]), torch.cat([c.reshape(-1) for c in preds])
    ws, out = hip.metrics_workspace(n, y.device), torch.zeros(5, dtype=torch.int64, device=DEV)
    stages = list(hip.METRICS_STAGES)
    for _ in range(2):
        hip.binary_metrics(p, y, workspace=ws, result=out, stages=stages)
    torch.cuda.synchronize()
    hip.enable_timing(True, only=("binary_metrics",))
    for _ in range(5):
        hip.binary_metrics(p, y, workspace=ws, result=out, stages=stages)
    torch.cuda.synchronize()
    meta = hip.timing_meta()
    res["launches"] = {k: {"calls": c, "ms": ms, "bytes": meta[k][0], "GB_per_s": meta[k][0] / ms * 1e-6,
                           "fraction_of_8TBps": meta[k][0] / (ms * 1e-3) / HBM_BYTES_PER_S}
                       for k, (c, ms) in hip.timing_summary().items() if k in meta}
    res["launches_ms_sum"] = sum(v["ms"] for v in res["launches"].values())
    hip.enable_timing(False)
    c = metrics.binary_counts(y, p)
    res["counts"] = {k: c[k] for k in ("two_u", "P", "N", "unsupported")}
    del labels, preds, y, p, ws
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[65536, 4194304, 45000000])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_epoch.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    lines = []
    for n in args.sizes:
        res = run(n, args.warmup, args.calls, args.host_repeats)
        if res is None:
            continue
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
