"""The additive-attention pooling of STAMP and ComirecSA (Fh.attention_pool), forward + backward over a batch of item rows
X [B, L, D] with a gradient arriving for out [B, K, D].  Two ways to the same outputs and the same gradients (X's, W1's, W2's
and the per-sample bias's), on the same box and the same data:

  composed  this project's CPU-path formulation run on device tensors (Fh.attention_pool_reference: two matmuls around the
            activation, the mask or the softmax, a batched matmul; Fh.attention_pool takes this path outside the kernel's
            limits).  It materialises the hidden tensor [B, L, Dh] and autograd keeps it for the backward.
  fused     one Fh.attention_pool node (csrc/attn_pool.hip).

Forms: "stamp" (sigmoid, mask, with the bias, Dh = D, K = 1) and "sa" (tanh, softmax, no bias, Dh and K as given).

Each side is timed with HIP events around `--calls` forward + backward iterations after `--warmup`, in `--rounds` rounds that
ALTERNATE the sides in one process (median, minimum and every round are reported); torch.cuda.max_memory_allocated of each
side is taken over one of its own iterations, above what the inputs and parameters hold (workspaces included: they come
from the same allocator).

    python profiles/microbench/attn_pool_step.py [--shapes stamp:4096x20x64x64x1 sa:4096x20x64x256x4 ...] [--out FILE]

Prints one JSON line per shape (form:B x L x D x Dh x K) and appends it to --out (default: attn_pool_step_mi355x.jsonl beside
this file).  Needs an MI355X: there is no CPU timing path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rec_pangu_amd import functional as Fh  # noqa: E402
from rec_pangu_amd import hip  # noqa: E402

DEV = "cuda"
FORMS = {"stamp": ("sigmoid", "mask", True), "sa": ("tanh", "softmax", False)}


def make_inputs(form, B, L, D, Dh, K, seed=1234):
    gen = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, L, D, generator=gen) * (2.0 / D) ** 0.5).to(DEV).requires_grad_(True)
    w1 = (torch.randn(D, Dh, generator=gen) * (1.0 / D) ** 0.5).to(DEV).requires_grad_(True)
    w2 = (torch.randn(Dh, K, generator=gen) * (1.0 / Dh) ** 0.5).to(DEV).requires_grad_(True)
    c = (torch.randn(B, Dh, generator=gen) * 0.5).to(DEV).requires_grad_(True) if FORMS[form][2] else None
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    valid = (torch.arange(L)[None, :] < lens[:, None]).float().to(DEV)
    g = torch.randn(B, K, D, generator=gen).to(DEV)
    return [x, w1, w2, c], valid, g


def clear(leaves):
    for t in leaves:
        if t is not None:
            t.grad = None


def composed_step(form, leaves, valid, g):
    clear(leaves)
    x, w1, w2, c = leaves
    out = Fh.attention_pool_reference(x, w1, w2, valid, c, FORMS[form][0], FORMS[form][1])
    out.backward(g)
    return out


def fused_step(form, leaves, valid, g):
    clear(leaves)
    x, w1, w2, c = leaves
    out = Fh.attention_pool(x, w1, w2, valid, bias=c, act=FORMS[form][0], norm=FORMS[form][1])
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
    clear(args[1])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step(*args)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run(form, B, L, D, Dh, K, warmup, calls, rounds):
    leaves, valid, g = make_inputs(form, B, L, D, Dh, K)
    args = (form, leaves, valid, g)
    res = {"form": form, "B": B, "L": L, "D": D, "Dh": Dh, "K": K, "warmup": warmup, "calls": calls, "rounds": rounds,
           "geometry": hip.attn_pool_geometry(), "fits": hip.attn_pool_fits(L, D, Dh, K), "bld_bytes": 4 * B * L * D,
           "hidden_bytes": 4 * B * L * Dh}
    clear(leaves)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    sides = {"composed": composed_step, "fused": fused_step}
    t0 = hip.torch_path_count()
    for name, fn in sides.items():
        for _ in range(warmup):
            fn(*args)
        res[f"{name}_max_memory_allocated"] = peak_of(fn, args, base)
    # what the forward alone leaves allocated for the backward
    for name in sides:
        clear(leaves)
        torch.cuda.synchronize()
        x, w1, w2, c = leaves
        if name == "composed":
            out = Fh.attention_pool_reference(x, w1, w2, valid, c, FORMS[form][0], FORMS[form][1])
        else:
            out = Fh.attention_pool(x, w1, w2, valid, bias=c, act=FORMS[form][0], norm=FORMS[form][1])
        torch.cuda.synchronize()
        res[f"{name}_held_after_forward"] = torch.cuda.memory_allocated() - base
        del out
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(timed(fn, args, calls))
    for name, ms in times.items():
        res[f"{name}_ms_median"], res[f"{name}_ms_min"], res[f"{name}_ms_all"] = statistics.median(ms), min(ms), ms
        res[f"{name}_spread"] = (max(ms) - min(ms)) / statistics.median(ms)
    res["composed_over_fused"] = res["composed_ms_median"] / res["fused_ms_median"]
    res["fused_over_composed_memory"] = res["fused_max_memory_allocated"] / res["composed_max_memory_allocated"]
    oc = composed_step(*args).detach().clone()
    gc = [None if t is None else t.grad.detach().clone() for t in leaves]
    of = fused_step(*args).detach().clone()
    torch.cuda.synchronize()
    res["out_max_abs"], res["out_max_abs_diff"] = float(oc.abs().max()), float((of - oc).abs().max())
    for name, t, ref in zip(("dx", "dw1", "dw2", "dc"), leaves, gc):
        if t is not None:
            res[f"{name}_max_abs"], res[f"{name}_max_abs_diff"] = float(ref.abs().max()), float((t.grad - ref).abs().max())
    res["fused_torch_paths"] = hip.torch_path_count() - t0

    # the launches one entry-point call at a time (a run of its own: the events serialise them)
    names = ("attn_pool_fwd", "attn_pool_bwd")
    hip.enable_timing(True, only=names)
    for _ in range(3):
        fused_step(*args)
    torch.cuda.synchronize()
    res["fused_launches"] = {k: {"calls": c, "ms": ms} for k, (c, ms) in hip.timing_summary().items()}
    hip.enable_timing(False)
    del args, leaves
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["stamp:4096x20x64x64x1", "stamp:4096x50x64x64x1", "sa:4096x20x64x256x4",
                                                    "sa:4096x50x64x256x4"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "attn_pool_step_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_pool_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    for shape in a.shapes:
        form, dims = shape.split(":")
        B, L, D, Dh, K = (int(x) for x in dims.split("x"))
        line = json.dumps(run(form, B, L, D, Dh, K, a.warmup, a.calls, a.rounds))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
