"""The session-graph encoder of SRGNN / NISER / GCSAN (models.layers.SRGNNCell.encode), forward + backward over a batch of
node rows H [B, L, D] and its alias lists, gradients arriving for seq_hidden [B, L, D] and ht [B, D].  Two ways to the same
outputs and the same gradients (H's and the cell's parameters'), on the same box and the same data:

  composed  this project's CPU-path formulation run on device tensors (Fh.ggnn_cell_reference: per step two Linears, gather /
            scatter_add over the transitions, lin_ih, lin_hh, the gates in torch ops; Fh.ggnn_cell takes this path outside the
            kernel's limits).  Its scatter_add uses float atomics on the device.
  fused     one Fh.ggnn_cell node per step (csrc/session_graph.hip).

The graph itself (rp_session_graph against Fh.session_graph_reference, the CPU path's batched torch ops, on the device) is
timed separately.

Each side is timed with HIP events around `--calls` forward + backward iterations after `--warmup`, in `--rounds` rounds that
ALTERNATE the sides in one process (median and minimum over the rounds are reported); torch.cuda.max_memory_allocated of each
side is taken over one of its own iterations, above what the inputs and parameters hold (workspaces included: they come
from the same allocator).

    python profiles/microbench/srgnn_step.py [--shapes 4096x20x64x1 4096x50x64x1 4096x20x64x2 4096x50x64x2] [--out FILE]

Prints one JSON line per shape (B x L x D x step) and appends it to --out (default: srgnn_step_mi355x.jsonl beside this file).
Needs an MI355X: there is no CPU timing path."""
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
from rec_pangu_amd.models.layers import SRGNNCell  # noqa: E402

DEV = "cuda"


def make_inputs(B, L, D, seed=1234):
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    cell = SRGNNCell(D)
    for p in cell.parameters():
        if p.dim() > 1:
            torch.nn.init.kaiming_normal_(p)
    cell = cell.to(DEV)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    hist = torch.randint(1, 4 * L, (B, L), generator=gen) * (torch.arange(L)[None, :] < lens[:, None])  # (repeats are common)
    hist = hist.to(DEV)
    alias = Fh.session_graph(hist)[1]
    h = torch.randn(B, L, D, generator=gen).to(DEV).requires_grad_(True)
    gs, gt = torch.randn(B, L, D, generator=gen).to(DEV), torch.randn(B, D, generator=gen).to(DEV)
    return cell, h, alias, gs, gt, hist


def clear(cell, h):
    h.grad = None
    for p in cell.parameters():
        p.grad = None


def composed_step(cell, h, alias, gs, gt, step):
    clear(cell, h)
    params = Fh._cell_params(cell)
    x = h
    for _ in range(step - 1):
        x = Fh.ggnn_cell_reference(x, alias, params, False)
    seq, ht = Fh.ggnn_cell_reference(x, alias, params, True)
    torch.autograd.backward([seq, ht], [gs, gt])
    return seq, ht


def fused_step(cell, h, alias, gs, gt, step):
    clear(cell, h)
    seq, ht = cell.encode(alias, h, step)
    torch.autograd.backward([seq, ht], [gs, gt])
    return seq, ht


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


def run(B, L, D, step, warmup, calls, rounds):
    cell, h, alias, gs, gt, hist = make_inputs(B, L, D)
    args = (cell, h, alias, gs, gt, step)
    res = {"B": B, "L": L, "D": D, "step": step, "warmup": warmup, "calls": calls, "rounds": rounds, "geometry": hip.ggnn_geometry(),
           "bld_bytes": 4 * B * L * D}
    clear(cell, h)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    sides = {"composed": composed_step, "fused": fused_step}
    t0 = hip.torch_path_count()
    for name, fn in sides.items():
        for _ in range(warmup):
            fn(*args)
        res[f"{name}_max_memory_allocated"] = peak_of(fn, args, base)
    times = {name: [] for name in sides}
    for _ in range(rounds):
        for name, fn in sides.items():
            times[name].append(timed(fn, args, calls))
    for name, ms in times.items():
        res[f"{name}_ms_median"], res[f"{name}_ms_min"], res[f"{name}_ms_all"] = statistics.median(ms), min(ms), ms
    res["composed_over_fused"] = res["composed_ms_median"] / res["fused_ms_median"]
    res["fused_over_composed_memory"] = res["fused_max_memory_allocated"] / res["composed_max_memory_allocated"]
    sc, tc = (t.detach().clone() for t in composed_step(*args))
    dc = h.grad.detach().clone()
    sf, tf = (t.detach().clone() for t in fused_step(*args))
    torch.cuda.synchronize()
    res["seq_max_abs"], res["seq_max_abs_diff"] = float(sc.abs().max()), float((sf - sc).abs().max())
    res["ht_max_abs_diff"], res["dh_max_abs_diff"] = float((tf - tc).abs().max()), float((h.grad - dc).abs().max())
    res["fused_torch_paths"] = hip.torch_path_count() - t0

    # the graph: one launch against the batched torch ops
    g_times = {"graph_kernel": [], "graph_torch": []}
    for fn_name, fn in (("graph_kernel", Fh.session_graph), ("graph_torch", Fh.session_graph_reference)):
        for _ in range(warmup):
            fn(hist)
    for _ in range(rounds):
        for fn_name, fn in (("graph_kernel", Fh.session_graph), ("graph_torch", Fh.session_graph_reference)):
            g_times[fn_name].append(timed(fn, (hist,), calls))
    for name, ms in g_times.items():
        res[f"{name}_ms_median"] = statistics.median(ms)
    assert all(torch.equal(a, b) for a, b in zip(Fh.session_graph(hist), Fh.session_graph_reference(hist)))

    # the launches one entry-point call at a time (a run of its own: the events serialise them)
    names = ("ggnn_cell_fwd", "ggnn_cell_bwd")
    hip.enable_timing(True, only=names)
    for _ in range(3):
        fused_step(*args)
    torch.cuda.synchronize()
    res["fused_launches"] = {k: {"calls": c, "ms": ms} for k, (c, ms) in hip.timing_summary().items()}
    hip.enable_timing(False)
    del args, cell, h
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x20x64x1", "4096x50x64x1", "4096x20x64x2", "4096x50x64x2"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "srgnn_step_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("srgnn_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    for shape in a.shapes:
        B, L, D, step = (int(x) for x in shape.split("x"))
        line = json.dumps(run(B, L, D, step, a.warmup, a.calls, a.rounds))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
