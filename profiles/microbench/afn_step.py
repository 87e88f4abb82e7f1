"""AFN's training step at the Criteo shape (26 sparse fields, D = 32, 5 logarithmic neurons, ensemble_dnn, both MLPs with the
reference's dropout of 0.1): the eager loop, the replayed step (GraphedTrainStep) and — as the baseline, not the code under
test — the same model with the logarithmic net composed from torch ops on the device (abs, clamp, log, nn.BatchNorm1d, the
Linear over the transposed tensor, exp, nn.BatchNorm1d, flatten: ATen kernels, every [B, F, D] intermediate held for autograd).
HIP events around `--steps` steps after `--warmup`; the block's own launch times and their fraction of 8 TB/s against the
algorithmic bytes (rows in + the MLP input out: forward; dout, z and rows in, dx out: backward) come from a separate short run
with per-launch events (hip.enable_timing).

    python profiles/microbench/afn_step.py [--batches 8192 65536] [--vocab-scale 16] [--out FILE]

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
from rec_pangu_amd.models.ranking import AFN  # noqa: E402
from rec_pangu_amd.optim import FusedAdam  # noqa: E402

DEV = "cuda"
BLOCK_ENTRY_POINTS = ("lognet_fwd", "lognet_bwd")
HBM_BYTES_PER_S = 8e12


def torch_block(rows, F, D, coefficient_W, log_bn, exp_bn, pad_to=64):
    """the block as the reference composes it (afn.py:93-102), from torch ops on the device (ATen kernels)"""
    E = rows[:, :F * D].reshape(rows.shape[0], F, D)
    y = log_bn(torch.log(torch.clamp(torch.abs(E), min=1e-5)))
    z = coefficient_W(y.transpose(2, 1)).transpose(1, 2)
    return torch.flatten(exp_bn(torch.exp(z)), start_dim=1)


def build(enc):
    torch.manual_seed(0)
    model = AFN(embedding_dim=32, enc_dict=enc).to(DEV)
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
    hip.enable_timing(True, only=BLOCK_ENTRY_POINTS)  # (events around every launch serialise the step: a run of its own)
    step = eager_step(model, opt)
    for i in range(10):
        step(i)
    torch.cuda.synchronize()
    meta = hip.timing_meta()
    res["block"] = {k: {"calls": n, "ms": ms, "bytes": meta[k][0], "GB_per_s": meta[k][0] / ms * 1e-6,
                        "fraction_of_8TBps": meta[k][0] / (ms * 1e-3) / HBM_BYTES_PER_S, "TFLOP_per_s": meta[k][1] / ms * 1e-9}
                    for k, (n, ms) in sorted(hip.timing_summary().items()) if k in meta}
    hip.enable_timing(False)
    del model, opt, step

    model, opt = build(enc)
    gstep = GraphedTrainStep(model, opt)
    res["replay_ms"] = timed(lambda i: gstep(batches[i % 8], batches[(i + 1) % 8]), warmup, steps)
    res["replay_backend"], res["why_not_plan"] = gstep.backend_used, gstep.why_not_plan
    del model, opt, gstep

    block = Fh.logarithmic_net
    Fh.logarithmic_net = torch_block
    try:
        model, opt = build(enc)
        res["torch_block_eager_ms"] = timed(eager_step(model, opt), warmup, steps)
    except Exception as e:  # the baseline may not fit or run at this size: written down, not fatal
        res["torch_block_eager_ms"] = None
        res["torch_block_eager_ms_error"] = f"{type(e).__name__}: {e}"[:300]
    finally:
        Fh.logarithmic_net = block
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
        raise SystemExit("afn_step.py times launches on an MI355X; no GPU is visible")
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
