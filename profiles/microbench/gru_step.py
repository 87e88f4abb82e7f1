"""The GRU encoder of GRU4Rec / NARM, forward + backward over a batch of id histories: a two-layer GRU with biases, H = D, every
row taking all L steps, a gradient arriving for the last hidden state (GRU4Rec's use).  Two ways to the same (H_all, h_last) and
the same gradients (the table's and every weight's), on the same box and the same data:

  fused     functional.gru_encode (csrc/gru.hip): the rows are gathered inside the first layer's launch, one recurrence launch
            per layer and direction, the weight gradients through the library's weight-gradient GEMM, the table's gradient
            through the sorted one-writer-per-row walk.
  composed  torch's own nn.GRU(batch_first=True) on the device behind F.embedding(ids, E, padding_idx=0), with autograd.

Both sides are timed with HIP events around `--calls` forward + backward iterations after `--warmup`, in `--rounds` rounds that
ALTERNATE the two sides in one process (median and minimum over the rounds are reported); torch.cuda.max_memory_allocated of
each side is taken over one of its own iterations, above what the inputs and parameters hold.

    python profiles/microbench/gru_step.py [--shapes 4096x20x64 4096x50x64 65536x20x32] [--out FILE]

Prints one JSON line per shape (B x L x D) and appends it to --out (default: gru_step_mi355x.jsonl beside this file).  Needs an
MI355X: there is no CPU timing path."""
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
V = 1 << 17
LAYERS = 2


def make_inputs(B, L, D, seed=1234):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    torch.manual_seed(seed)
    rnn = torch.nn.GRU(D, D, LAYERS, batch_first=True).to(DEV)
    for p in rnn.parameters():
        if p.dim() == 2:
            torch.nn.init.kaiming_normal_(p)  # as the models' reset_parameters leaves them
    E = (torch.randn(V, D, device=DEV, generator=gen) * (2.0 / D) ** 0.5).requires_grad_(True)
    ids = torch.randint(1, V, (B, L), device=DEV, generator=gen)
    steps = torch.full((B,), L, dtype=torch.int32, device=DEV)
    g_last = torch.randn(B, D, device=DEV, generator=gen)
    return rnn, E, ids, steps, g_last


def clear(rnn, E):
    E.grad = None
    for p in rnn.parameters():
        p.grad = None


def fused_step(rnn, E, ids, steps, g_last):
    clear(rnn, E)
    _, h_last = Fh.gru_encode(rnn, steps, steps - 1, ids=ids, item_weight=E, packed=False, check_indices="deferred")
    h_last.backward(g_last)
    return h_last


def composed_step(rnn, E, ids, steps, g_last):
    clear(rnn, E)
    out, _ = rnn(torch.nn.functional.embedding(ids, E, padding_idx=0))
    h_last = out[:, -1]
    h_last.backward(g_last)
    return h_last


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


def run(B, L, D, warmup, calls, rounds):
    args = make_inputs(B, L, D)
    rnn, E = args[0], args[1]
    res = {"B": B, "L": L, "D": D, "H": D, "layers": LAYERS, "V": V, "warmup": warmup, "calls": calls, "rounds": rounds,
           "geometry": hip.gru_geometry(), "workspace_bytes": hip.gru_workspace_bytes(B, L, D, D, True),
           "saved_hidden_bytes": 4 * LAYERS * B * L * D}
    clear(rnn, E)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    sides = {"fused": fused_step, "composed": composed_step}
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
    res["composed_over_fused"] = res["composed_ms_median"] / res["fused_ms_median"]
    hf, hc = fused_step(*args).detach(), composed_step(*args).detach()
    res["h_last_max_abs_diff"] = float((hf - hc).abs().max())

    # the launches one entry-point call at a time (a run of its own: the events serialise them)
    hip.enable_timing(True, only=("gru_fwd", "gru_bwd", "hist_rows_bwd"))
    for _ in range(3):
        fused_step(*args)
    torch.cuda.synchronize()
    res["launches"] = {k: {"calls": c, "ms": ms} for k, (c, ms) in hip.timing_summary().items()}
    hip.enable_timing(False)
    del args, rnn, E
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4096x20x64", "4096x50x64", "65536x20x32"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "gru_step_mi355x.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_step.py times launches on an MI355X; no GPU is visible")
    hip.lib()
    for shape in a.shapes:
        B, L, D = (int(x) for x in shape.split("x"))
        line = json.dumps(run(B, L, D, a.warmup, a.calls, a.rounds))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
