"""The multi-interest encoder of ComirecDR and of MIND, forward + backward over a batch of gathered history rows X [B, L, D]
with a padded tail, a gradient arriving for the [B, K, D] interests.  Two ways to the same interests and the same gradients
(X's and the projection's), on the same box and the same data:

  fused     models.layers.CapsuleNetwork on the device (csrc/capsule.hip): ComirecDR's projection as one launch for all
            positions (no [B, L, K D, D] product), MIND's through the library's Linear, the three routing rounds as one launch
            each way.
  composed  the reference's formulation in torch on the device, op for op (rec_pangu/models/layers/multi_interest.py:96-156):
            sum(w * x.unsqueeze(2), dim=3) or linear + repeat, reshape / transpose / contiguous, about twenty small ops per
            routing round, with autograd.  Where it runs out of memory that is recorded as its result.

Both sides are timed with HIP events around `--calls` forward + backward iterations after `--warmup`, in `--rounds` rounds that
ALTERNATE the two sides in one process (median and minimum over the rounds are reported); torch.cuda.max_memory_allocated of
each side is taken over one of its own iterations, above what the inputs and parameters hold.  MIND's initial logits are
drawn once and fed to both sides.

    python profiles/microbench/capsule_step.py [--shapes 4096x20x4x64 4096x50x4x64 65536x20x4x32] [--out FILE]

Prints one JSON line per encoder and shape (B x L x K x D) and appends it to --out (default: capsule_step_mi355x.jsonl beside
this file).  Needs an MI355X: there is no CPU timing path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rec_pangu_amd import functional as Fh, hip  # noqa: E402
from rec_pangu_amd.models.layers import CapsuleNetwork  # noqa: E402

DEV = "cuda"
ENCODERS = {"ComirecDR": 2, "MIND": 0}


def make_inputs(btype, B, L, K, D, seed=1234):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    torch.manual_seed(seed)
    layer = CapsuleNetwork(D, L, bilinear_type=btype, interest_num=K)
    for p in layer.parameters():
        torch.nn.init.normal_(p, std=(2.0 / D) ** 0.5)  # (projected rows of the inputs' size, interests of O(0.1))
    layer = layer.to(DEV)
    x = (torch.randn(B, L, D, device=DEV, generator=gen) * (2.0 / D) ** 0.5).requires_grad_(True)
    lens = torch.randint(1, L + 1, (B,), device=DEV, generator=gen)
    mask = (torch.arange(L, device=DEV)[None, :] < lens[:, None]).long()
    b0 = torch.randn(B, K, L, device=DEV, generator=gen)
    layer.initial_logits = lambda batch, device: b0
    g = torch.randn(B, K, D, device=DEV, generator=gen)
    return layer, x, mask, b0, g


def clear(layer, x):
    x.grad = None
    for p in layer.parameters():
        p.grad = None


def fused_step(layer, x, mask, b0, g):
    clear(layer, x)
    out = layer(x, mask, DEV)
    out.backward(g)
    return out


def composed_step(layer, x, mask, b0, g):
    clear(layer, x)
    K, L = layer.interest_num, layer.seq_len
    if layer.bilinear_type == 0:
        u_hat, logits = torch.nn.functional.linear(x, layer.linear.weight), b0
    else:
        u_hat, logits = torch.sum(layer.w[:, :L, :, :] * torch.unsqueeze(x, dim=2), dim=3), None
    out = Fh._capsule_route_torch(u_hat, mask, K, logits, layer.bilinear_type == 0, False)
    out.backward(g)
    return out


def timed(step, args, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def peak_of(step, args, base):
    clear(args[0], args[1])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step(*args)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run(encoder, B, L, K, D, warmup, calls, rounds):
    btype = ENCODERS[encoder]
    args = make_inputs(btype, B, L, K, D)
    layer, x = args[0], args[1]
    res = {"encoder": encoder, "B": B, "L": L, "K": K, "D": D, "warmup": warmup, "calls": calls, "rounds": rounds,
           "geometry": hip.capsule_geometry(), "projected_rows_bytes": 4 * B * L * D * (K if btype else 1),
           "product_bytes": 4 * B * L * K * D * D if btype else 0}
    clear(layer, x)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    sides = {"fused": fused_step, "composed": composed_step}
    t0 = hip.torch_path_count()
    for name, step in list(sides.items()):
        try:
            for _ in range(warmup):
                step(*args)
            res[f"{name}_max_memory_allocated"] = peak_of(step, args, base)
        except torch.cuda.OutOfMemoryError:
            res[f"{name}_result"] = "out of memory"
            del sides[name]
            clear(layer, x)
            torch.cuda.empty_cache()
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, step in sides.items():
            times[name].append(timed(step, args, calls))
    for name, ms in times.items():
        res[f"{name}_ms_median"], res[f"{name}_ms_min"], res[f"{name}_ms_all"] = statistics.median(ms), min(ms), ms
    if len(sides) == 2:
        res["composed_over_fused"] = res["composed_ms_median"] / res["fused_ms_median"]
        of, oc = fused_step(*args).detach(), composed_step(*args).detach()
        res["interests_max_abs"], res["interests_max_abs_diff"] = float(oc.abs().max()), float((of - oc).abs().max())
    res["fused_torch_paths"] = hip.torch_path_count() - t0

    # the launches one entry-point call at a time (a run of its own: the events serialise them)
    names = ("capsule_project_fwd", "capsule_project_bwd_x", "capsule_project_bwd_w", "capsule_route_fwd", "capsule_route_bwd",
             "linear_fwd", "linear_wgrad")
    hip.enable_timing(True, only=names)
    for _ in range(3):
        fused_step(*args)
    torch.cuda.synchronize()
    res["launches"] = {k: {"calls": c, "ms": ms} for k, (c, ms) in hip.timing_summary().items()}
    hip.enable_timing(False)
    del args, layer, x
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x20x4x64", "4096x50x4x64", "65536x20x4x32"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "capsule_step_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("capsule_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    for shape in a.shapes:
        B, L, K, D = (int(x) for x in shape.split("x"))
        for encoder in ENCODERS:
            line = json.dumps(run(encoder, B, L, K, D, a.warmup, a.calls, a.rounds))
            print(line, flush=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
