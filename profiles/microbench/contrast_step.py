"""The in-batch contrastive loss of CLRec and ContraRec (Fh.contrastive_loss), forward + backward, and one training step of
each model.  Two ways to the same numbers, on the same box and the same data:

  composed  this project's CPU-path formulation run on device tensors (Fh.contrastive_loss_reference: the [n, m] matrix
            several times over, kept by autograd; Fh.contrastive_loss takes this path outside the kernel's limits);
  fused     one Fh.contrastive_loss node (csrc/contrast.hip).

Loss shapes: "clrec:n x m x d" (a against b, labels arange, scale 1, T = 0.1) and "contrarec:n x d" (symmetric, n / 2
distinct targets drawn from 1000 values twice over, the self pair excluded, scale = T = 0.2).
Step shapes: "step:<model>:B x V x D x L" -- forward, backward and the fused Adam step of models.sequence.CLRec / ContraRec
(BERT4Rec encoder), against the same model with Fh.contrastive_loss and the key-padding Fh.seq_attention forced onto their
composed torch formulations (everything else stays on the library's kernels on both sides).

Each side is timed with HIP events around `--calls` iterations after `--warmup`, in `--rounds` rounds that ALTERNATE the sides
in one process (median, minimum and every round are reported); what the forward leaves allocated for the backward and
torch.cuda.max_memory_allocated over one iteration are taken above what the inputs hold.

    python profiles/microbench/contrast_step.py [--shapes clrec:4096x4096x64 contrarec:8192x64 step:clrec:4096x50000x64x20 ...]

Prints one JSON line per shape and appends it to --out (default: contrast_step_mi355x.jsonl beside this file).  Needs an
MI355X: there is no CPU timing path."""
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
_FUSED = {"contrastive_loss": Fh.contrastive_loss, "seq_attention": Fh.seq_attention}


def _composed_loss(a, b, la, lb, temperature, exclude_self=False, scale=1.0):
    return Fh.contrastive_loss_reference(a, b, la, lb, temperature, exclude_self, scale)


def _composed_attention(qkv, mask, heads, p=0.0, training=False, qpos=None, q=None, causal=True):
    if causal:
        return _FUSED["seq_attention"](qkv, mask, heads, p, training, qpos, q, causal)
    D = qkv.shape[1] // (3 if q is None else 2)
    qr, kv = (qkv[:, :D], qkv[:, D:]) if q is None else (q, qkv)
    return Fh.seq_attention_reference(qr, kv, mask, heads, qpos=qpos, compact=q is not None, causal=False)


def use(side):
    """route the models' calls: "fused" the library's kernels, "composed" the torch formulations of the two new pieces"""
    Fh.contrastive_loss = _FUSED["contrastive_loss"] if side == "fused" else _composed_loss
    Fh.seq_attention = _FUSED["seq_attention"] if side == "fused" else _composed_attention


def timed(step, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(res, sides, warmup, calls, rounds, forward_only=None):
    """sides: {name: step()}; forward_only: {name: fn() -> output} for the memory held after the forward"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for name, fn in sides.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        res[f"{name}_max_memory_allocated"] = torch.cuda.max_memory_allocated() - base
    for name, fn in (forward_only or {}).items():
        torch.cuda.synchronize()
        out = fn()
        torch.cuda.synchronize()
        res[f"{name}_held_after_forward"] = torch.cuda.memory_allocated() - base
        del out
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(timed(fn, calls))
    for name, ms in times.items():
        res[f"{name}_ms_median"], res[f"{name}_ms_min"], res[f"{name}_ms_all"] = statistics.median(ms), min(ms), ms
        res[f"{name}_spread"] = (max(ms) - min(ms)) / statistics.median(ms)
    res["composed_over_fused"] = res["composed_ms_median"] / res["fused_ms_median"]


def run_loss(form, dims, warmup, calls, rounds):
    gen = torch.Generator().manual_seed(1234)
    if form == "clrec":
        n, m, d = dims
        T, excl, scale = 0.1, False, 1.0
        b = torch.nn.functional.normalize(torch.randn(m, d, generator=gen), dim=-1).to(DEV).requires_grad_(True)
        la, lb = torch.arange(n, device=DEV), torch.arange(m, device=DEV)
    else:
        n, d = dims
        m, T, excl, scale, b, lb = n, 0.2, True, 0.2, None, None
        la = torch.randint(0, 1000, (n // 2,), generator=gen).repeat(2).to(DEV)
    a = torch.nn.functional.normalize(torch.randn(n, d, generator=gen), dim=-1).to(DEV).requires_grad_(True)
    leaves = [t for t in (a, b) if t is not None]
    res = {"form": form, "n": n, "m": m, "d": d, "T": T, "warmup": warmup, "calls": calls, "rounds": rounds,
           "geometry": hip.contrast_geometry(), "fits": hip.contrast_fits(d), "matrix_bytes": 4 * n * m,
           "workspace_bytes": hip.contrast_workspace_bytes(n, m, d)}

    def step(fn):
        def go():
            for t in leaves:
                t.grad = None
            loss = fn(a, b, la, lb, T, excl, scale)
            loss.backward()
            return loss
        return go

    sides = {"composed": step(_composed_loss), "fused": step(_FUSED["contrastive_loss"])}
    fwd = {"composed": lambda: _composed_loss(a, b, la, lb, T, excl, scale),
           "fused": lambda: _FUSED["contrastive_loss"](a, b, la, lb, T, excl, scale)}
    t0 = hip.torch_path_count()
    measure(res, sides, warmup, calls, rounds, fwd)
    lc = sides["composed"]().detach().clone()
    gc = [t.grad.detach().clone() for t in leaves]
    lf = sides["fused"]().detach().clone()
    torch.cuda.synchronize()
    res["loss"], res["loss_abs_diff"] = float(lc), abs(float(lf) - float(lc))
    for name, t, ref in zip(("da", "db"), leaves, gc):
        res[f"{name}_max_abs"], res[f"{name}_max_abs_diff"] = float(ref.abs().max()), float((t.grad - ref).abs().max())
    res["fused_torch_paths"] = hip.torch_path_count() - t0
    names = ("contrast_fwd", "contrast_bwd")
    hip.enable_timing(True, only=names)
    for _ in range(3):
        sides["fused"]()
    torch.cuda.synchronize()
    res["fused_launches"] = {k: {"calls": c, "ms": ms} for k, (c, ms) in hip.timing_summary().items()}
    hip.enable_timing(False)
    return res


def run_step(model_name, dims, warmup, calls, rounds):
    from rec_pangu_amd.models import sequence
    from rec_pangu_amd.optim import make_adam
    B, V, D, L = dims
    gen = torch.Generator().manual_seed(1234)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    mask = (torch.arange(L)[None, :] < lens[:, None]).long()
    batch = {"hist_item_list": (torch.randint(1, V - 1, (B, L), generator=gen) * mask).to(DEV), "hist_mask_list": mask.to(DEV),
             "target_item": torch.randint(1, V, (B, 1), generator=gen).to(DEV)}
    cls = {"clrec": sequence.CLRec, "contrarec": sequence.ContraRec}[model_name]
    torch.manual_seed(3)
    model = cls({"item_id": {"vocab_size": V}}, {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id",
                                                 "cate_cols": []}).to(DEV).train()
    model.check_indices = "deferred"
    opt = make_adam(model, 1e-3)
    res = {"form": f"step:{model_name}", "B": B, "V": V, "D": D, "L": L, "warmup": warmup, "calls": calls, "rounds": rounds}

    def step(side):
        def go():
            use(side)
            try:
                torch.manual_seed(7)  # the same augmentations on both sides
                model(batch)["loss"].backward()
                opt.step()
                model.zero_grad()
            finally:
                use("fused")
        return go

    measure(res, {"composed": step("composed"), "fused": step("fused")}, warmup, calls, rounds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["clrec:4096x4096x64", "contrarec:8192x64", "step:clrec:4096x50000x64x20",
                                                    "step:clrec:4096x50000x64x50", "step:contrarec:4096x50000x64x20",
                                                    "step:contrarec:4096x50000x64x50"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "contrast_step_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrast_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    torch.matmul(torch.ones(8, 8, device=DEV), torch.ones(8, 8, device=DEV))  # (the BLAS workspace: allocated once, 160 MB)
    torch.cuda.synchronize()
    for shape in a.shapes:
        parts = shape.split(":")
        dims = tuple(int(x) for x in parts[-1].split("x"))
        if parts[0] == "step":
            res = run_step(parts[1], dims, a.warmup, a.calls, a.rounds)
        else:
            res = run_loss(parts[0], dims, a.warmup, a.calls, a.rounds)
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
