#!/usr/bin/env python
"""SASRec golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_sasrec.py

  model_sasrec_train.npz     rec_pangu/models/sequence/sasrec.py: n_layers 2, n_heads 2, inner_size 16, both dropouts 0, train
                             mode, 'gelu'
  model_sasrec_eval.npz      the defaults (2 layers, 4 heads, inner_size 32, both dropouts 0.1, 'gelu') under model.eval()
  model_sasrec_l1_relu.npz   n_layers 1, n_heads 1, inner_size default, both dropouts 0, train mode, 'relu': the layer that
                             runs in last-row mode on the device is the only layer

Item vocabulary V = 37, embedding_dim D = 8, max_length L = 6, the hand-made batch of B = 5 of make_golden_gru.py (GRU4Rec's
form): a padded tail (row 0, length 4), a full-length row with an id 0 inside it (row 1), a length-3 row (2), a full-length row
(3), a length-1 row (4), a repeated target (4 twice) and the targets 0 and V - 1; no empty row (the reference raises there).
Groups init/ batch/ out/ grad/ adam2/ adam2_out/ as make_golden_seq.dump_model writes them; two Adam steps at lr = 1e-2.

Seed choice (the discipline of make_golden_seq.py): per file the model seed is the FIRST from 1234 upward at which the
reference in fp32 and a float64 copy of it, stepped side by side, agree within a TENTH of the bars the tests use
(tests/test_sasrec_host.py = tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, with 1e-6 as the other tolerance,
the tighter of the two readings per element) on out, grad, adam2 and adam2_out; adam2 leaves the key biases out (see
KEY_BIAS below).  The encoder's float32 rounding sits near a tenth of the `out` bar, so the search is longer than the GRU
files' was.  Printed by the run that wrote the committed fixtures (the first and the accepted line of each file; every seed
between them was rejected in the same way, 94 lines in all):

  sasrec_train: seed 1234: fp32-f64 over bar/10: out 2.9 grad 0.8 adam2 0.2 adam2_out 4.6 | rejected
  sasrec_train: seed 1246: fp32-f64 over bar/10: out 0.7 grad 0.8 adam2 0.094 adam2_out 0.83 | ok
  sasrec_eval: seed 1234: fp32-f64 over bar/10: out 1.1 grad 1.5 adam2 0.11 adam2_out 1.5 | rejected
  sasrec_eval: seed 1299: fp32-f64 over bar/10: out 0.82 grad 0.43 adam2 0.22 adam2_out 0.58 | ok
  sasrec_l1_relu: seed 1234: fp32-f64 over bar/10: out 1.7 grad 0.65 adam2 0.14 adam2_out 1.8 | rejected
  sasrec_l1_relu: seed 1245: fp32-f64 over bar/10: out 0.8 grad 0.45 adam2 0.049 adam2_out 0.98 | ok

Only data is written: no reference source, bytecode or pickled reference objects.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

_ref_import.install()

from rec_pangu.models.sequence import SASRec  # noqa: E402

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
BARS = {"out": (1e-5, 1e-6), "grad": (1e-4, 1e-6), "adam2": (1e-4, 1e-6), "adam2_out": (1e-5, 1e-6)}  # (big, small)
# The gradient of every key bias is ZERO in exact arithmetic: q_i . (k_j + b) shifts all scores of a row by q_i . b and the
# softmax does not see it.  The reference's fp32 gradient there is rounding noise near 1e-9 (its float64 copy: 1e-17), which Adam
# normalises into steps of up to lr: after two steps fp32 and float64 differ by 1e4 bars in those entries at EVERY seed, and
# nothing that computes in floating point reproduces them.  They stay in the files as the reference wrote them; the seed search
# and the tests leave them out of adam2 (the tests bound their distance from init/ by Adam's step instead).  The model's output
# does not depend on them, so adam2_out is compared in full.
KEY_BIAS = "multi_head_attention.key.bias"
NO_DROP = {"hidden_dropout_prob": 0.0, "attn_dropout_prob": 0.0}
CASES = {
    "sasrec_train": dict(config=dict(NO_DROP, n_layers=2, n_heads=2, inner_size=16), train=True),
    "sasrec_eval": dict(config={}, train=False),
    "sasrec_l1_relu": dict(config=dict(NO_DROP, n_layers=1, n_heads=1, hidden_act="relu"), train=True),
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
    model = SASRec(ENC, dict(CONFIG, **case["config"]))
    return model.train() if case["train"] else model.eval()


def adam(model):
    return torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)


def worst(group, got, want):
    """largest |fp32 - f64| over a tenth of the bar; the bar is the tighter of (atol, rtol) = (big, 1e-6) and (1e-6, big)"""
    big, small = BARS[group]
    w = 0.0
    for k, v in want.items():
        if group == "adam2" and k.endswith(KEY_BIAS):
            continue
        v = v.detach()
        bar = torch.minimum(big + small * v.abs(), small + big * v.abs())
        w = max(w, float(((got[k].detach().double() - v).abs() / (bar / 10)).max()))
    return w


def check(name, case, seed):
    torch.manual_seed(seed)
    m32 = build(case)
    m64 = copy.deepcopy(m32).double()
    opts = [adam(m32), adam(m64)]
    data = batch()
    agree = {}
    for step in range(3):
        if step == 2:
            with torch.no_grad():
                agree["adam2_out"] = worst("adam2_out", m32(data, is_training=False), m64(data, is_training=False))
            break
        r32, r64 = m32(data), m64(data)
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
    ok = max(agree.values()) <= 1.0
    print(f"  {name}: seed {seed}: fp32-f64 over bar/10: " + " ".join(f"{k} {v:.2g}" for k, v in agree.items()) +
          (" | ok" if ok else " | rejected"))
    return ok


def dump_model(name, case, seed):
    out = {"seed": np.asarray(seed)}
    data = batch()
    torch.manual_seed(seed)
    model = build(case)
    for k, v in model.state_dict().items():
        out["init/" + k] = to_np(v)
    for k, v in data.items():
        out["batch/" + k] = to_np(v)
    res = model(data)
    for k, v in res.items():
        out["out/" + k] = to_np(v)
    model.zero_grad()
    res["loss"].backward()
    for k, p in model.named_parameters():
        out["grad/" + k] = to_np(p.grad)
    torch.manual_seed(seed)
    model = build(case)
    opt = adam(model)
    for _ in range(2):
        model(data)["loss"].backward()
        opt.step()
        model.zero_grad()
    for k, v in model.state_dict().items():
        out["adam2/" + k] = to_np(v)
    with torch.no_grad():
        for k, v in model(data, is_training=False).items():
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
