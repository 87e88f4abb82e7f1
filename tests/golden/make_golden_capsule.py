#!/usr/bin/env python
"""MIND / ComirecDR golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_capsule.py

  model_mind_train.npz   rec_pangu/models/sequence/mind.py (CapsuleNetwork, bilinear_type 0, random initial logits), train mode
  model_mind_eval.npz    the same after model.eval() (the reference draws the logits in evaluation too)
  model_comirecdr.npz    rec_pangu/models/sequence/comirec.py:67-118 (bilinear_type 2, zero initial logits)

Item vocabulary V = 37, embedding_dim D = 8, max_length L = 6, K = 3 interests, a hand-made batch of B = 5 (the YotubeDNN
fixture's shape): a padded tail (row 0, length 4), a full-length row with an id 0 inside it (row 1), a length-3 row (2), a
full-length row (3), a length-1 row (4), a repeated target (4 twice) and the targets 0 and V - 1.  No fully masked row: it
gives v = 0 for every interest and so an exact tie in the readout; that case is tested at kernel level.  Groups init/
batch/ out/ grad/ adam2/ adam2_out/ as make_golden_gru.dump_model writes them (a parameter without a gradient —
capsule.relu.0.weight, unused with relu_layer off — has no grad/ entry); two Adam steps at lr = 1e-2.

MIND draws its initial routing logits torch.randn(B, K, L) inside every forward.  logits/out, logits/adam2_0, logits/adam2_1
and logits/adam2_out record them per forward, in the order dump_model calls the model: read off the generator's state in
front of the call, the state put back, so the reference itself draws the same numbers.  The device test feeds them.

Seed choice (the discipline of make_golden_gru.py): per file the model seed is the FIRST from 1234 upward at which the
reference in fp32 and a float64 copy of it, stepped side by side on the same draws, agree within a TENTH of the bars the
tests use (tests/test_capsule_host.py = tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, with 1e-6 as the other
tolerance, the tighter of the two readings per element) on out, grad, adam2 and adam2_out — AND at which, in float64, the
two best readout scores of every row of both training forwards are at least 1e-3 max|score| apart: below that an fp32
rounding could flip the chosen interest, and with it the loss and every gradient.  (The float64 copy runs with torch.rand /
torch.randn returning the float32 draws cast up and torch.zeros returning float64: the reference writes the chosen interest
into a torch.rand placeholder and starts the routing from fp32 logits, which a float64 model does not accept.)
Printed by the run that wrote the committed fixtures:

  mind_train: seed 1234: fp32-f64 over bar/10: out 0.41 grad 0.18 adam2 0.014 adam2_out 0.82 | top-two gap 0.00072 | rejected
  mind_train: seed 1235: fp32-f64 over bar/10: out 0.23 grad 0.066 adam2 0.02 adam2_out 0.34 | top-two gap 5e-05 | rejected
  mind_train: seed 1236: fp32-f64 over bar/10: out 0.56 grad 0.1 adam2 0.045 adam2_out 0.65 | top-two gap 0.0055 | ok
  mind_eval: seed 1234: fp32-f64 over bar/10: out 0.41 grad 0.18 adam2 0.014 adam2_out 0.82 | top-two gap 0.00072 | rejected
  mind_eval: seed 1235: fp32-f64 over bar/10: out 0.23 grad 0.066 adam2 0.02 adam2_out 0.34 | top-two gap 5e-05 | rejected
  mind_eval: seed 1236: fp32-f64 over bar/10: out 0.56 grad 0.1 adam2 0.045 adam2_out 0.65 | top-two gap 0.0055 | ok
  comirecdr: seed 1234: fp32-f64 over bar/10: out 0.0066 grad 0.0096 adam2 0.29 adam2_out 0.029 | top-two gap 0.028 | ok

Only data is written: no reference source, bytecode or pickled reference objects.
"""
import contextlib
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

_ref_import.install()

from rec_pangu.models.sequence import MIND, ComirecDR  # noqa: E402

V, D, L, K = 37, 8, 6, 3
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": [], "K": K}
BARS = {"out": (1e-5, 1e-6), "grad": (1e-4, 1e-6), "adam2": (1e-4, 1e-6), "adam2_out": (1e-5, 1e-6)}  # (big, small)
GAP = 1e-3
CASES = {
    "mind_train": dict(cls=MIND, train=True, logits=True),
    "mind_eval": dict(cls=MIND, train=False, logits=True),
    "comirecdr": dict(cls=ComirecDR, train=True, logits=False),
}


def to_np(t):
    return t.detach().cpu().numpy()


def batch():
    hist = torch.tensor([[3, 7, 7, 12, 0, 0],
                         [5, 0, 9, 36, 1, 2],
                         [4, 9, 11, 0, 0, 0],
                         [36, 35, 34, 33, 32, 31],
                         [7, 0, 0, 0, 0, 0]], dtype=torch.long)
    mask = torch.tensor([[1, 1, 1, 1, 0, 0],
                         [1, 1, 1, 1, 1, 1],
                         [1, 1, 1, 0, 0, 0],
                         [1, 1, 1, 1, 1, 1],
                         [1, 0, 0, 0, 0, 0]], dtype=torch.long)
    target = torch.tensor([[4], [20], [4], [0], [V - 1]], dtype=torch.long)
    return {"hist_item_list": hist, "hist_mask_list": mask, "target_item": target}


def build(case):
    model = case["cls"](ENC, dict(CONFIG))
    return model.train() if case["train"] else model.eval()


def adam(model):
    return torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)


@contextlib.contextmanager
def draws_as_float64():
    """torch.rand / torch.randn return the same float32 draws, cast to float64, and torch.zeros (ComirecDR's initial logits)
    float64 zeros, while the float64 copy runs"""
    rand, randn, zeros = torch.rand, torch.randn, torch.zeros
    torch.rand = lambda *a, **k: rand(*a, **k).double()
    torch.randn = lambda *a, **k: randn(*a, **k).double()
    torch.zeros = lambda *a, **k: zeros(*a, **k).double()
    try:
        yield
    finally:
        torch.rand, torch.randn, torch.zeros = rand, randn, zeros


def peek_logits():
    """the torch.randn(B, K, L) the next forward will draw; the generator's state is put back"""
    state = torch.get_rng_state()
    logits = torch.randn(5, K, L)
    torch.set_rng_state(state)
    return logits


def both(m32, m64, data, **kw):
    """the two models on the same draws"""
    state = torch.get_rng_state()
    r32 = m32(data, **kw)
    torch.set_rng_state(state)
    with draws_as_float64():
        r64 = m64(data, **kw)
    return r32, r64


def worst(group, got, want):
    """largest |fp32 - f64| over a tenth of the bar; the bar is the tighter of (atol, rtol) = (big, 1e-6) and (1e-6, big)"""
    big, small = BARS[group]
    w = 0.0
    for k, v in want.items():
        if v is None:
            continue
        v = v.detach()
        bar = torch.minimum(big + small * v.abs(), small + big * v.abs())
        w = max(w, float(((got[k].detach().double() - v).abs() / (bar / 10)).max()))
    return w


def readout_gap(m64, r64, data):
    """smallest (best - second best readout score) / max|score| over the rows, in float64"""
    e = m64.item_emb.weight.detach()[data["target_item"].view(-1)]
    s = torch.bmm(r64["user_emb"].detach(), e.unsqueeze(-1)).squeeze(-1)
    top = torch.sort(s, dim=1, descending=True).values
    return float(((top[:, 0] - top[:, 1]) / s.abs().max()).min())


def check(name, case, seed):
    torch.manual_seed(seed)
    m32 = build(case)
    m64 = copy.deepcopy(m32).double()
    opts = [adam(m32), adam(m64)]
    data = batch()
    agree, gap = {}, float("inf")
    for step in range(3):
        if step == 2:
            with torch.no_grad():
                agree["adam2_out"] = worst("adam2_out", *both(m32, m64, data, is_training=False))
            break
        r32, r64 = both(m32, m64, data)
        gap = min(gap, readout_gap(m64, r64, data))
        r32["loss"].backward(), r64["loss"].backward()
        if step == 0:
            agree["out"] = worst("out", r32, r64)
            agree["grad"] = worst("grad", {k: p.grad for k, p in m32.named_parameters()},
                                  {k: p.grad for k, p in m64.named_parameters()})
        for o, m in zip(opts, (m32, m64)):
            o.step()
            m.zero_grad()
        if step == 1:
            agree["adam2"] = worst("adam2", m32.state_dict(), m64.state_dict())
    ok = max(agree.values()) <= 1.0 and gap >= GAP
    print(f"  {name}: seed {seed}: fp32-f64 over bar/10: " + " ".join(f"{k} {v:.2g}" for k, v in agree.items()) +
          f" | top-two gap {gap:.2g}" + (" | ok" if ok else " | rejected"))
    return ok


def dump_model(name, case, seed):
    out = {"seed": np.asarray(seed)}
    data = batch()

    def forward(model, tag, **kw):
        if case["logits"]:
            out["logits/" + tag] = to_np(peek_logits())
        return model(data, **kw)

    torch.manual_seed(seed)
    model = build(case)
    for k, v in model.state_dict().items():
        out["init/" + k] = to_np(v)
    for k, v in data.items():
        out["batch/" + k] = to_np(v)
    res = forward(model, "out")
    for k, v in res.items():
        out["out/" + k] = to_np(v)
    model.zero_grad()
    res["loss"].backward()
    for k, p in model.named_parameters():
        if p.grad is not None:
            out["grad/" + k] = to_np(p.grad)
    torch.manual_seed(seed)
    model = build(case)
    opt = adam(model)
    for step in range(2):
        forward(model, f"adam2_{step}")["loss"].backward()
        opt.step()
        model.zero_grad()
    for k, v in model.state_dict().items():
        out["adam2/" + k] = to_np(v)
    with torch.no_grad():
        for k, v in forward(model, "adam2_out", is_training=False).items():
            out["adam2_out/" + k] = to_np(v)
    np.savez_compressed(os.path.join(HERE, f"model_{name}.npz"), **out)
    print(f"wrote model_{name}.npz", len(out), "arrays")


if __name__ == "__main__":
    for name, case in CASES.items():
        seed = 1234
        while not check(name, case, seed):
            seed += 1
            assert seed < 1234 + 2000, "no seed found"
        dump_model(name, case, seed)
