"""AITM's training step with the default constructor at the Criteo shape (26 sparse fields, D = 32: towers of 832 -> 400 -> 400
-> 400, attention over T = 2 tokens of width 400): the eager loop, the replayed step (GraphedTrainStep) and — as the baseline, not
the code under test — the same model with the two forms this script is about switched off: hip.attention_wide_fits patched to
False (the attention layer then composes itself from torch ops on the device, a counted torch path) and Fh.pair_loss replaced by
the loss written with torch ops (two sigmoids, two BCELosses, maximum, sum).  HIP events around `--steps` steps after `--warmup`;
the new launches' own times and their fraction of 8 TB/s against the algorithmic bytes (attention forward: 4 T a 4 B read and
a 4 B written per sample) come from a separate short run with per-launch events (hip.enable_timing).

    python profiles/microbench/aitm_step.py [--batches 8192 65536] [--vocab-scale 16] [--out FILE]

Prints one JSON line per batch size.  Needs an MI355X: there is no CPU timing path."""
import argparse
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench import criteo_enc_dict, synth_batch  # noqa: E402
from rec_pangu_amd import functional as Fh, hip  # noqa: E402
from rec_pangu_amd.graph_step import GraphedTrainStep  # noqa: E402
from rec_pangu_amd.models.multi_task import AITM  # noqa: E402
from rec_pangu_amd.optim import FusedAdam  # noqa: E402

DEV = "cuda"
NEW_ENTRY_POINTS = ("attention_wide_fwd", "attention_wide_bwd", "pair_loss_fwd", "pair_loss_bwd")
HBM_BYTES_PER_S = 8e12


def torch_pair_loss(z1, z2, y1, y2, mode, coef, apply_sigmoid=True):
    """AITM's loss as the reference composes it (aitm.py:84-100), from torch ops on the device (ATen kernels)"""
    assert mode == hip.PAIR_AITM
    p1, p2 = (torch.sigmoid(z1), torch.sigmoid(z2)) if apply_sigmoid else (z1, z2)
    bce = torch.nn.functional.binary_cross_entropy
    loss = bce(p1, y1) + bce(p2, y2) + coef * torch.sum(torch.maximum(p2 - p1, torch.zeros_like(y1)))
    return p1, p2, loss


def build(enc):
    torch.manual_seed(0)
    model = AITM(enc_dict=enc).to(DEV)
    for m in model.modules():
        if hasattr(m, "check_indices"):
            m.check_indices = "deferred"
    model.train()
    opt = FusedAdam(model.parameters(), lr=1e-3, fuse_zero_grad=True, lazy_tables=True, replay="closed", defer=True)
    return model, opt


def timed(step, warmup, steps):
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(warmup, warmup + steps):
        step(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def run(B, enc, warmup, steps):
    batches = [synth_batch(enc, B, 100 + i, DEV) for i in range(8)]
    res = {"batch": B, "warmup": warmup, "steps": steps}

    def eager_step(model, opt):
        def step(i):
            model.prefetch(batches[(i + 1) % 8])
            out = model(batches[i % 8])
            out["loss"].backward()
            opt.step()
            model.zero_grad()
        return step

    model, opt = build(enc)
    n_paths = hip.torch_path_count()
    res["eager_ms"] = timed(eager_step(model, opt), warmup, steps)
    res["torch_paths_in_the_step"] = hip.torch_path_count() - n_paths
    hip.enable_timing(True, only=NEW_ENTRY_POINTS)  # (events around every launch serialise the step: a run of its own)
    step = eager_step(model, opt)
    for i in range(10):
        step(i)
    torch.cuda.synchronize()
    meta = hip.timing_meta()
    res["launches"] = {k: {"calls": n, "ms": ms, **({"bytes": meta[k][0], "GB_per_s": meta[k][0] / ms * 1e-6,
                                                     "fraction_of_8TBps": meta[k][0] / (ms * 1e-3) / HBM_BYTES_PER_S}
                                                    if k in meta else {})}
                       for k, (n, ms) in sorted(hip.timing_summary().items())}
    hip.enable_timing(False)
    del model, opt, step

    model, opt = build(enc)
    gstep = GraphedTrainStep(model, opt)
    res["replay_ms"] = timed(lambda i: gstep(batches[i % 8], batches[(i + 1) % 8]), warmup, steps)
    res["replay_backend"], res["why_not_plan"] = gstep.backend_used, gstep.why_not_plan
    del model, opt, gstep

    fits, loss = hip.attention_wide_fits, Fh.pair_loss
    hip.attention_wide_fits, Fh.pair_loss = (lambda T, H, a: False), torch_pair_loss
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)  # (the counted torch path of the composed attention)
            model, opt = build(enc)
            n_paths = hip.torch_path_count()
            res["forms_off_eager_ms"] = timed(eager_step(model, opt), warmup, steps)
            res["forms_off_torch_paths_per_step"] = (hip.torch_path_count() - n_paths) / (warmup + steps)
            del model, opt
            model, opt = build(enc)
            gstep = GraphedTrainStep(model, opt)
            res["forms_off_replay_ms"] = timed(lambda i: gstep(batches[i % 8], batches[(i + 1) % 8]), warmup, steps)
            res["forms_off_replay_backend"] = gstep.backend_used
            del model, opt, gstep
    except Exception as e:  # the baseline may not run at this size: written down, not fatal
        res["forms_off_error"] = f"{type(e).__name__}: {e}"[:300]
    finally:
        hip.attention_wide_fits, Fh.pair_loss = fits, loss
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--vocab-scale", type=int, default=16, help="divide every Criteo cardinality")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aitm_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    enc = criteo_enc_dict(args.vocab_scale)
    lines = []
    for B in args.batches:
        res = run(B, enc, args.warmup, args.steps)
        res["vocab_scale"], res["matmul"] = args.vocab_scale, hip.get_matmul_precision()
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
