"""The loss head of the sequence-recall family, forward + backward: CrossEntropyLoss over the whole item vocabulary of
scores = U @ E.T.  Two ways to the same loss and the same two gradients, on the same box and the same data:

  fused     functional.full_softmax_ce (csrc/softmax_ce.hip): no [B, V] tensor; forward (main + finish + mean), dU (main + split
            reduce) and dE launches.
  composed  the reference's own formulation on the device: F.cross_entropy(U @ E.T, t) with autograd, which keeps the logits,
            the softmax and their gradient ([B, V] each).  Skipped, with the reason, where those three tensors do not fit the
            free device memory.

Both sides are timed with HIP events around `--calls` forward + backward iterations after `--warmup`, in `--rounds` rounds that
ALTERNATE the two sides in one process (median and minimum over the rounds are reported); torch.cuda.max_memory_allocated of
each side is taken over its own iterations, above what the inputs hold.  The matrix-core share is the fused side's algorithmic
flops (forward 2 BVD, dU and dE 4 BVD each: the score tile is recomputed by both) times the bf16 products per flop the launch
ran (6 in the automatic mode) over its time, against 2.5 PFLOP/s dense bf16.  Per-launch times come from a separate short run
under hip.enable_timing (events around every entry-point call serialise them).

    python profiles/microbench/seq_ce_step.py [--shapes 4096x131072x64 4096x1048576x64 65536x131072x64] [--out FILE]

Prints one JSON line per shape.  Needs an MI355X: there is no CPU timing path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rec_pangu_amd import functional as Fh, hip  # noqa: E402

DEV = "cuda"
PEAK_BF16 = 2.5e15
PRODUCTS = 6  # csrc/softmax_ce.hip: the automatic precision mode runs the fp32-faithful six for every D it takes


def make_inputs(B, V, D, seed=1234):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    E = (torch.randn(V, D, device=DEV, generator=gen) * (2.0 / D) ** 0.5).requires_grad_(True)  # kaiming, as the model inits
    U = (torch.randn(B, D, device=DEV, generator=gen) * 0.5).requires_grad_(True)
    t = torch.randint(0, V, (B,), device=DEV, generator=gen)
    return U, E, t


def fused_step(U, E, t):
    U.grad = E.grad = None
    loss = Fh.full_softmax_ce(U, E, t, check_indices="deferred")
    loss.backward()
    return loss


def composed_step(U, E, t):
    U.grad = E.grad = None
    loss = torch.nn.functional.cross_entropy(torch.matmul(U, E.transpose(1, 0)), t)
    loss.backward()
    return loss


def timed(step, args, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def peak_of(step, args, base):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step(*args)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run(B, V, D, warmup, calls, rounds):
    U, E, t = make_inputs(B, V, D)
    args = (U, E, t)
    res = {"B": B, "V": V, "D": D, "warmup": warmup, "calls": calls, "rounds": rounds, "products": PRODUCTS,
           "splits": hip.softmax_ce_splits(B, V), "workspace_bytes": hip.softmax_ce_workspace_bytes(B, V, D),
           "logits_bytes": 4 * B * V}
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    free, _ = torch.cuda.mem_get_info()
    need = 3 * 4 * B * V + 4 * (B + V) * D * 2
    composed = need < 0.9 * free
    if not composed:
        res["composed_skipped"] = (f"the logits, the softmax and their gradient need {need / 2 ** 30:.0f} GiB, "
                                   f"{free / 2 ** 30:.0f} GiB of device memory are free")
    sides = {"fused": fused_step}
    if composed:
        sides["composed"] = composed_step
    for name, step in sides.items():
        for _ in range(warmup):
            step(*args)
        res[f"{name}_max_memory_allocated"] = peak_of(step, args, base)
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, step in sides.items():
            times[name].append(timed(step, args, calls))
    for name, ms in times.items():
        res[f"{name}_ms_median"], res[f"{name}_ms_min"], res[f"{name}_ms_all"] = statistics.median(ms), min(ms), ms
    flops = 10.0 * B * V * D
    res["fused_algorithmic_flops"] = flops
    res["fused_matrix_core_share"] = flops * PRODUCTS / (res["fused_ms_median"] * 1e-3) / PEAK_BF16
    if composed:
        res["composed_over_fused"] = res["composed_ms_median"] / res["fused_ms_median"]
        lf, lc = float(fused_step(*args).detach()), float(composed_step(*args).detach())
        res["loss_fused"], res["loss_composed"] = lf, lc

    # the launches one entry-point call at a time (a run of its own: the events serialise them)
    hip.enable_timing(True, only=("softmax_ce_fwd", "softmax_ce_bwd"))
    for _ in range(3):
        fused_step(*args)
    torch.cuda.synchronize()
    meta = hip.timing_meta()
    res["launches"] = {k: {"calls": c, "ms": ms, "flops": meta[k][1],
                           "matrix_core_share": meta[k][1] * PRODUCTS / (ms * 1e-3) / PEAK_BF16}
                       for k, (c, ms) in hip.timing_summary().items() if k in meta}
    res["launches_ms_sum"] = sum(v["ms"] for v in res["launches"].values())
    hip.enable_timing(False)
    del U, E, t, args
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x131072x64", "4096x1048576x64", "65536x131072x64"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seq_ce_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    lines = []
    for shape in a.shapes:
        B, V, D = (int(x) for x in shape.split("x"))
        lines.append(json.dumps(run(B, V, D, a.warmup, a.calls, a.rounds)))
        print(lines[-1], flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
