"""AOANet's training step at the Criteo shape (26 sparse + 13 dense, D = 32, the default 3 interaction layers over 4
subspaces, trunk [64, 64, 64]): the eager loop, the replayed step (GraphedTrainStep) and — as the baseline, not the code under
test — the same model with its interaction net on the FACTORISED einsums over stock torch ops.  (The reference's own
formulation, the [B, 676, 32, 32] outer product, is 2.8 MB per sample: 180 GB at batch 65536, it cannot run at these sizes.)
HIP events around `--steps` steps after `--warmup`; the interaction launches' own times, flop/s and bytes/s come from a
separate short run with per-launch events (hip.enable_timing).

    python profiles/microbench/aoanet_step.py [--batches 8192 65536] [--vocab-scale 16] [--out FILE]

Prints one JSON line per batch size.  Needs an MI355X: there is no CPU timing path."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from bench import criteo_enc_dict, synth_batch  # noqa: E402
from rec_pangu_amd import functional as Fh, hip  # noqa: E402
from rec_pangu_amd.graph_step import GraphedTrainStep  # noqa: E402
from rec_pangu_amd.models.ranking import AOANet  # noqa: E402
from rec_pangu_amd.optim import FusedAdam  # noqa: E402

DEV = "cuda"
GIN_ENTRY_POINTS = ("gin_fwd", "gin_bwd")


def torch_stack(rows, F, D, layers):
    """the net as GeneralizedInteraction.factorised composes it from torch ops, here on the device (ATen kernels)"""
    B0 = rows[:, :F * D].reshape(rows.shape[0], F, D)
    Bi = B0
    for layer in layers:
        Bi = layer.factorised(B0, Bi)
    return Bi.flatten(start_dim=1)


def build(enc):
    torch.manual_seed(0)
    model = AOANet(embedding_dim=32, enc_dict=enc).to(DEV)
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
    res["eager_ms"] = timed(eager_step(model, opt), warmup, steps)
    hip.enable_timing(True, only=GIN_ENTRY_POINTS)  # (events around every launch serialise the step: a run of its own)
    step = eager_step(model, opt)
    for i in range(10):
        step(i)
    torch.cuda.synchronize()
    meta = hip.timing_meta()
    res["gin"] = {k: {"calls": n, "ms": ms, "GB_per_s": meta[k][0] / ms * 1e-6, "TFLOP_per_s": meta[k][1] / ms * 1e-9}
                  for k, (n, ms) in sorted(hip.timing_summary().items()) if k in meta}
    hip.enable_timing(False)
    del model, opt, step

    model, opt = build(enc)
    gstep = GraphedTrainStep(model, opt)
    res["replay_ms"] = timed(lambda i: gstep(batches[i % 8], batches[(i + 1) % 8]), warmup, steps)
    res["replay_backend"], res["why_not_plan"] = gstep.backend_used, gstep.why_not_plan
    del model, opt, gstep

    stack, Fh.gin_stack = Fh.gin_stack, torch_stack
    try:
        model, opt = build(enc)
        res["torch_stack_eager_ms"] = timed(eager_step(model, opt), warmup, steps)
    finally:
        Fh.gin_stack = stack
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[8192, 65536])
    ap.add_argument("--vocab-scale", type=int, default=16, help="divide every Criteo cardinality (the dense blocks do not depend on it)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aoanet_step.py times launches on an MI355X; no GPU is visible")
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
