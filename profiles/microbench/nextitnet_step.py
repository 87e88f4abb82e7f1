"""NextItNet's encoder (models.layers.NextItNetLayer), forward + backward over a batch of gathered history rows X [B, L, D] with
a padded tail, a gradient arriving for the one row per sample the model reads, [B, D].  Three ways to the same row and the
same gradients (X's and the encoder's parameters'), on the same box and the same data, feat_drop off:

  composed  the reference's formulation in torch on the device, op for op (rec_pangu/models/layers/conv.py): masked_fill,
            transpose to [B, C, L], per conv a left pad and a library convolution, the channel LayerNorm from var_mean, ReLU,
            the residual; then the indexed row.  (Fh.causal_conv_block takes this path outside the kernel's limits.)
  full      the fused block launches (csrc/causal_conv.hip) with the final block forced to full mode, then Fh.seq_take.
  last      the layer as the model runs it: every block but the final one in full mode, the final one in last mode.

Each side is timed with HIP events around `--calls` forward + backward iterations after `--warmup`, in `--rounds` rounds that
ALTERNATE the sides in one process (median and minimum over the rounds are reported); torch.cuda.max_memory_allocated of each
side is taken over one of its own iterations, above what the inputs and parameters hold (workspaces included: they come
from the same allocator).

    python profiles/microbench/nextitnet_step.py [--shapes 4096x20x64x0 4096x50x64x0 4096x20x64x1 4096x50x64x1] [--out FILE]

Prints one JSON line per shape (B x L x D x one_masked; dilations and kernel_size the reference's defaults) and appends it to
--out (default: nextitnet_step_mi355x.jsonl beside this file).  Needs an MI355X: there is no CPU timing path."""
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
from rec_pangu_amd.models.layers import NextItNetLayer  # noqa: E402

DEV = "cuda"


def make_inputs(B, L, D, one_masked, seed=1234):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    torch.manual_seed(seed)
    layer = NextItNetLayer(D, None, bool(one_masked), 3)
    for p in layer.parameters():
        if p.dim() > 1:
            torch.nn.init.kaiming_normal_(p)  # (NextItNet.reset_parameters: gamma and beta too)
    layer = layer.to(DEV)
    x = torch.randn(B, L, D, device=DEV, generator=gen).requires_grad_(True)
    lens = torch.randint(1, L + 1, (B,), device=DEV, generator=gen)
    g = torch.randn(B, D, device=DEV, generator=gen)
    return layer, x, lens, g


def clear(layer, x):
    x.grad = None
    for p in layer.parameters():
        p.grad = None


def composed_step(layer, x, lens, g):
    clear(layer, x)
    B, L, _ = x.shape
    behind = torch.arange(L, device=x.device).unsqueeze(0).expand(B, L) >= lens.unsqueeze(-1)
    y = torch.masked_fill(x, behind.unsqueeze(-1), 0).transpose(1, 2)
    for block in layer.res_blocks:
        y = block(y)
    out = y[torch.arange(B, device=x.device), :, lens - 1]
    out.backward(g)
    return out


def full_step(layer, x, lens, g):
    clear(layer, x)
    layer.last_mode = False
    out = layer(x, lens)
    out.backward(g)
    return out


def last_step(layer, x, lens, g):
    clear(layer, x)
    layer.last_mode = True
    out = layer(x, lens)
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


def run(B, L, D, one_masked, warmup, calls, rounds):
    args = make_inputs(B, L, D, one_masked)
    layer, x = args[0], args[1]
    res = {"B": B, "L": L, "D": D, "one_masked": one_masked, "dilations": [b.dilation for b in layer.res_blocks], "kernel_size": 3,
           "warmup": warmup, "calls": calls, "rounds": rounds, "geometry": hip.causal_conv_geometry(), "blc_bytes": 4 * B * L * D}
    clear(layer, x)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    sides = {"composed": composed_step, "full": full_step, "last": last_step}
    t0 = hip.torch_path_count()
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
    res["composed_over_full"] = res["composed_ms_median"] / res["full_ms_median"]
    res["composed_over_last"] = res["composed_ms_median"] / res["last_ms_median"]
    res["full_over_last"] = res["full_ms_median"] / res["last_ms_median"]
    oc = composed_step(*args).detach().clone()
    of = full_step(*args).detach().clone()
    ol = last_step(*args).detach().clone()
    torch.cuda.synchronize()
    res["row_max_abs"] = float(oc.abs().max())
    res["full_max_abs_diff"], res["last_max_abs_diff"] = float((of - oc).abs().max()), float((ol - oc).abs().max())
    res["fused_torch_paths"] = hip.torch_path_count() - t0

    # the launches one entry-point call at a time (a run of its own: the events serialise them)
    names = ("causal_conv_fwd", "causal_conv_bwd", "seq_take_fwd", "seq_take_bwd")
    for side, step in (("full", full_step), ("last", last_step)):
        hip.enable_timing(True, only=names)
        for _ in range(3):
            step(*args)
        torch.cuda.synchronize()
        res[f"{side}_launches"] = {k: {"calls": c, "ms": ms} for k, (c, ms) in hip.timing_summary().items()}
        hip.enable_timing(False)
    del args, layer, x
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x20x64x0", "4096x50x64x0", "4096x20x64x1", "4096x50x64x1"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "nextitnet_step_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nextitnet_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    for shape in a.shapes:
        B, L, D, one_masked = (int(x) for x in shape.split("x"))
        line = json.dumps(run(B, L, D, one_masked, a.warmup, a.calls, a.rounds))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
