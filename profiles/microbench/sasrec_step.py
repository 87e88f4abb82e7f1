"""SASRec's TransformerEncoder, forward + backward over a batch of gathered history rows X [B, L, D] with a padded tail, a
gradient arriving for the one row per sample the model reads, [B, D].  Three ways to the same row and the same gradients (X's
and the encoder's parameters'), on the same box and the same data, dropouts off:

  composed  the reference's formulation in torch on the device, op for op (rec_pangu/models/layers/trainformer.py): three
            projections, permutes, the [B, heads, L, L] scores, additive mask, softmax, P V, permute / contiguous, dense,
            LayerNorm, the feed-forward; then gather_indexes.  (models.layers.TransformerEncoder takes this path for a
            [B, 1, L, L] additive mask.)
  full      models.layers.TransformerEncoder on the device with the [B, L] content mask: per layer one stacked Q | K | V GEMM and
            the fused attention launch each way (csrc/seq_attn.hip), every layer over all B L rows; then gather_indexes.
  last      TransformerEncoder.encode_last: the same, with the final layer in last-row mode (K and V for all positions, Q, the
            attention row, dense, both LayerNorms and the feed-forward for B rows).

Each side is timed with HIP events around `--calls` forward + backward iterations after `--warmup`, in `--rounds` rounds that
ALTERNATE the sides in one process (median and minimum over the rounds are reported); torch.cuda.max_memory_allocated of each
side is taken over one of its own iterations, above what the inputs and parameters hold.

    python profiles/microbench/sasrec_step.py [--shapes 4096x20x64x4 4096x50x64x4] [--layers 2] [--out FILE]

Prints one JSON line per shape (B x L x D x heads) and appends it to --out (default: sasrec_step_mi355x.jsonl beside this
file).  Needs an MI355X: there is no CPU timing path."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from rec_pangu_amd import hip  # noqa: E402
from rec_pangu_amd.models.layers import TransformerEncoder  # noqa: E402
from rec_pangu_amd.models.layers.transformer import additive_attention_mask  # noqa: E402

DEV = "cuda"


def make_inputs(B, L, D, heads, layers, seed=1234):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    torch.manual_seed(seed)
    enc = TransformerEncoder(n_layers=layers, n_heads=heads, hidden_size=D, inner_size=32, hidden_dropout_prob=0.0,
                             attn_dropout_prob=0.0, hidden_act="gelu", layer_norm_eps=1e-3)
    for p in enc.parameters():
        if p.dim() > 1:
            torch.nn.init.kaiming_normal_(p)  # (SASRec.reset_parameters)
    enc = enc.to(DEV)
    x = torch.randn(B, L, D, device=DEV, generator=gen).requires_grad_(True)
    lens = torch.randint(1, L + 1, (B,), device=DEV, generator=gen)
    mask = (torch.arange(L, device=DEV)[None, :] < lens[:, None]).long()
    g = torch.randn(B, D, device=DEV, generator=gen)
    return enc, x, mask, additive_attention_mask(mask), lens - 1, g


def clear(enc, x):
    x.grad = None
    for p in enc.parameters():
        p.grad = None


def gathered(out, last):
    return out.gather(dim=1, index=last.view(-1, 1, 1).expand(-1, -1, out.shape[-1])).squeeze(1)


def composed_step(enc, x, mask, add, last, g):
    clear(enc, x)
    out = gathered(enc(x, add, output_all_encoded_layers=False)[-1], last)
    out.backward(g)
    return out


def full_step(enc, x, mask, add, last, g):
    clear(enc, x)
    out = gathered(enc(x, mask, output_all_encoded_layers=False)[-1], last)
    out.backward(g)
    return out


def last_step(enc, x, mask, add, last, g):
    clear(enc, x)
    out = enc.encode_last(x, mask)
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


def run(B, L, D, heads, layers, warmup, calls, rounds):
    args = make_inputs(B, L, D, heads, layers)
    enc, x = args[0], args[1]
    res = {"B": B, "L": L, "D": D, "heads": heads, "layers": layers, "warmup": warmup, "calls": calls, "rounds": rounds,
           "geometry": hip.seq_attn_geometry(), "scores_bytes": 4 * B * heads * L * L}
    clear(enc, x)
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
    oc = composed_step(*args).detach().clone()
    of = full_step(*args).detach().clone()
    ol = last_step(*args).detach().clone()
    torch.cuda.synchronize()
    res["row_max_abs"] = float(oc.abs().max())
    res["full_max_abs_diff"], res["last_max_abs_diff"] = float((of - oc).abs().max()), float((ol - oc).abs().max())
    res["composed_torch_paths_per_step"] = layers
    t1 = hip.torch_path_count()
    full_step(*args), last_step(*args)
    res["fused_torch_paths"] = hip.torch_path_count() - t1
    assert hip.torch_path_count() - t0 > 0  # (the composed side is the counted path)

    # the launches one entry-point call at a time (a run of its own: the events serialise them)
    names = ("seq_attn_fwd", "seq_attn_bwd", "seq_act_fwd", "seq_act_bwd", "linear_fwd", "linear_wgrad", "layernorm_fwd",
             "layernorm_bwd")
    for side, step in (("full", full_step), ("last", last_step)):
        hip.enable_timing(True, only=names)
        for _ in range(3):
            step(*args)
        torch.cuda.synchronize()
        res[f"{side}_launches"] = {k: {"calls": c, "ms": ms} for k, (c, ms) in hip.timing_summary().items()}
        hip.enable_timing(False)
    del args, enc, x
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x20x64x4", "4096x50x64x4"])
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "sasrec_step_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sasrec_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    warnings.simplefilter("ignore", RuntimeWarning)  # (the composed side is the counted torch path, on purpose)
    for shape in a.shapes:
        B, L, D, heads = (int(x) for x in shape.split("x"))
        line = json.dumps(run(B, L, D, heads, a.layers, a.warmup, a.calls, a.rounds))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
