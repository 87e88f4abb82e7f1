#!/usr/bin/env python
"""NextItNet golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_nextitnet.py

  model_nextitnet_default.npz     rec_pangu/models/sequence/nextitnet.py, the default config: two-masked blocks, dilations
                                  None -> [1, 4], kernel_size 3.  At L = 6 the convs of dilation 4 and 8 read padding through
                                  every tap but the last (and, at dilation 4, the one before it for positions >= 4): those
                                  weight gradients are exactly zero and Adam leaves the entries where they were
  model_nextitnet_d12_k2.npz      two-masked, dilations [1, 2], kernel_size 2: every tap is live
  model_nextitnet_one_masked.npz  one_masked True, dilations [1, 2], kernel_size 3: the middle width is 4

Item vocabulary V = 37, embedding_dim D = 8, max_length L = 6, the GRU4Rec fixture's hand-made batch of B = 5 (a padded
tail, a full-length row with an id 0 inside it, a full-length row, a length-1 row, a repeated target, the targets 0 and
V - 1), all in train mode (feat_drop 0).  Groups init/ batch/ out/ grad/ adam2/ adam2_out/ as make_golden_gru.dump_model writes
them; two Adam steps at lr = 1e-2.  `fc.weight` is created and never used: it has no gradient and is left out of grad/; its
adam2/ equals init/.  model_nextitnet_default.npz also holds batch2/ out2/ grad2/: the same batch with row 2 emptied (the
reference defines it: position L - 1 of an all-zero input), forward and gradients of the freshly built model.

Seed choice (the discipline of make_golden_seq.py): per file the model seed is the FIRST from 1234 upward at which the
reference in fp32 and a float64 copy of it, stepped side by side, agree within a TENTH of the bars the tests use
(tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, with 1e-6 as the other tolerance, the tighter of the two
readings per element) on out, grad, adam2 and adam2_out (and out2, grad2 where written).  Printed by the run that wrote the
committed fixtures:

  nextitnet_default: seed 1234: fp32-f64 over bar/10: out2 0.4 grad2 0.17 out 0.35 grad 0.16 adam2 0.052 adam2_out 0.72 | ok
  nextitnet_d12_k2: seed 1234: fp32-f64 over bar/10: out 0.33 grad 0.19 adam2 0.091 adam2_out 0.15 | ok
  nextitnet_one_masked: seed 1234: fp32-f64 over bar/10: out 0.29 grad 0.19 adam2 0.017 adam2_out 1.2 | rejected
  nextitnet_one_masked: seed 1235: fp32-f64 over bar/10: out 0.53 grad 0.65 adam2 0.17 adam2_out 0.97 | ok

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

from rec_pangu.models.sequence import NextItNet  # noqa: E402

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
BARS = {"out": (1e-5, 1e-6), "grad": (1e-4, 1e-6), "adam2": (1e-4, 1e-6), "adam2_out": (1e-5, 1e-6)}  # (big, small)
CASES = {
    "nextitnet_default": dict(config={}, empty=True),
    "nextitnet_d12_k2": dict(config={"dilations": [1, 2], "kernel_size": 2}, empty=False),
    "nextitnet_one_masked": dict(config={"one_masked": True, "dilations": [1, 2], "kernel_size": 3}, empty=False),
}


def to_np(t):
    return t.detach().cpu().numpy()


def batch(empty=False):
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
    if empty:
        hist[2] = 0
        mask[2] = 0
    target = torch.tensor([[4], [20], [4], [0], [V - 1]], dtype=torch.long)
    return {"hist_item_list": hist, "hist_mask_list": mask, "target_item": target}


def build(case):
    return NextItNet(ENC, dict(CONFIG, **case["config"])).train()


def adam(model):
    return torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)


def worst(group, got, want):
    """largest |fp32 - f64| over a tenth of the bar; the bar is the tighter of (atol, rtol) = (big, 1e-6) and (1e-6, big)"""
    big, small = BARS[group]
    w = 0.0
    for k, v in want.items():
        v = v.detach()
        bar = torch.minimum(big + small * v.abs(), small + big * v.abs())
        w = max(w, float(((got[k].detach().double() - v).abs() / (bar / 10)).max()))
    return w


def grads_of(model):
    return {k: p.grad for k, p in model.named_parameters() if p.grad is not None}


def check(name, case, seed):
    torch.manual_seed(seed)
    m32 = build(case)
    m64 = copy.deepcopy(m32).double()
    agree = {}
    if case["empty"]:
        data2 = batch(True)
        r32, r64 = m32(data2), m64(data2)
        r32["loss"].backward(), r64["loss"].backward()
        agree["out2"] = worst("out", r32, r64)
        agree["grad2"] = worst("grad", grads_of(m32), grads_of(m64))
        m32.zero_grad(), m64.zero_grad()
    opts = [adam(m32), adam(m64)]
    data = batch()
    for step in range(3):
        if step == 2:
            with torch.no_grad():
                agree["adam2_out"] = worst("adam2_out", m32(data, is_training=False), m64(data, is_training=False))
            break
        r32, r64 = m32(data), m64(data)
        r32["loss"].backward(), r64["loss"].backward()
        if step == 0:
            agree["out"] = worst("out", r32, r64)
            assert set(grads_of(m32)) == set(dict(m32.named_parameters())) - {"fc.weight"}
            agree["grad"] = worst("grad", grads_of(m32), grads_of(m64))
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
    for k, g in grads_of(model).items():
        out["grad/" + k] = to_np(g)
    if case["empty"]:
        data2 = batch(True)
        for k, v in data2.items():
            out["batch2/" + k] = to_np(v)
        model.zero_grad()
        res = model(data2)
        for k, v in res.items():
            out["out2/" + k] = to_np(v)
        res["loss"].backward()
        for k, g in grads_of(model).items():
            out["grad2/" + k] = to_np(g)
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
