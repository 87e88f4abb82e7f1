#!/usr/bin/env python
"""ESSM / AITM golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_mtl.py

  model_essm_eval.npz    rec_pangu/models/multi_task/essm.py:12-75, embedding_dim=8, hidden_dim=[8, 4], dropouts=[0.2, 0.2],
                         eval mode (dropout inactive)
  model_essm_train.npz   the same with dropouts=[0, 0] (the MLPs then hold no Dropout module), train mode
  model_aitm_eval.npz    rec_pangu/models/multi_task/aitm.py:14-100, embedding_dim=8, tower_dims=[16, 8, 12],
                         drop_prob=[0.1, 0.1, 0.1], eval mode
  model_aitm_train.npz   the same with drop_prob=[0, 0, 0], train mode
on make_golden.py's small schema and batch (5 sparse features, B = 24, task1_label / task2_label).  Groups init/ batch/ out/
grad/ adam2/ adam2_out/ as make_golden.dump_model_case writes them (no BatchNorm: no after1/ entries).  Predictions are
[24, 1] for ESSM and [24] for AITM; every parameter receives a gradient (asserted).

Seed choice.  ReLUs and AITM's max(p2 - p1, 0) are kinks: where the argument is closer to 0 than two fp32 implementations'
rounding difference, they may disagree about the side.  The generator evaluates, in float64, at the three states every fixture
records (the initial weights, after the first and after the second Adam step): every ReLU pre-activation (the towers,
info_layer, the attention output before its ReLU) and, for AITM, p2 - p1 of every row.  It takes the FIRST model seed from 1234
upward at which, in all four cases, every one of them is at least 1e-5 in magnitude and each side of AITM's constraint holds at
least 3 of the 24 rows.  It prints the seed; the tests build their models with it (tests/test_mtl_host.py: SEED).
Only data is written: no reference source, bytecode or pickled reference objects.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import shim; its generators only run under __main__)

from rec_pangu.models.multi_task import ESSM, AITM  # noqa: E402

MARGIN = 1e-5
MIN_SIDE = 3
CASES = {  # name -> (class, constructor arguments, train mode)
    "essm_eval": (ESSM, dict(embedding_dim=8, hidden_dim=[8, 4], dropouts=[0.2, 0.2]), False),
    "essm_train": (ESSM, dict(embedding_dim=8, hidden_dim=[8, 4], dropouts=[0.0, 0.0]), True),
    "aitm_eval": (AITM, dict(embedding_dim=8, tower_dims=[16, 8, 12], drop_prob=[0.1, 0.1, 0.1]), False),
    "aitm_train": (AITM, dict(embedding_dim=8, tower_dims=[16, 8, 12], drop_prob=[0.0, 0.0, 0.0]), True),
}


def build(name):
    cls, kw, _ = CASES[name]
    return cls(enc_dict=G.small_enc_dict(), **kw)


def margins(model, data):
    """(smallest |ReLU pre-activation|, smallest |p2 - p1|, rows with p2 > p1) of a float64 copy of the model on the batch;
    the last two are (inf, None) for ESSM"""
    m64 = copy.deepcopy(model).double()
    m64.eval()  # (the recorded states have no active dropout: eval mode, or rates of 0)
    d64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in data.items()}
    pre = []
    hooks = [mod.register_forward_hook(lambda _m, inp, _out: pre.append(inp[0].detach().abs().min()))
             for mod in m64.modules() if isinstance(mod, torch.nn.ReLU)]
    att = getattr(m64, "attention_layer", None)
    if att is not None:
        def before_the_attention_relu(_m, inp, _out):
            x = inp[0]
            p = torch.softmax(torch.einsum("bta,bsa->bts", att.W_q(x), att.W_k(x)), dim=2)
            pre.append((torch.einsum("bts,bsa->bta", p, att.W_v(x)) + x).detach().abs().min())
        hooks.append(att.register_forward_hook(before_the_attention_relu))
    with torch.no_grad():
        out = m64(d64, is_training=False)
    for h in hooks:
        h.remove()
    n_relu = sum(isinstance(mod, torch.nn.ReLU) for mod in m64.modules()) + (att is not None)
    assert len(pre) == n_relu, "a ReLU was not reached"
    gap, above = float("inf"), None
    if att is not None:
        diff = out["task2_pred"] - out["task1_pred"]
        gap, above = float(diff.abs().min()), int((diff > 0).sum())
    return float(min(pre)), gap, above


def recorded_states_ok(name, seed):
    _, _, train_mode = CASES[name]
    torch.manual_seed(seed)
    model = build(name)
    model.train(train_mode)
    data = G.small_batch()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    ok, seen = True, []
    for step in range(3):
        relu, gap, above = margins(model, data)
        seen.append(f"{relu:.3g}" + ("" if above is None else f" (|p2-p1| {gap:.3g}, {above} rows above)"))
        ok = ok and relu >= MARGIN and gap >= MARGIN and (above is None or MIN_SIDE <= above <= G.B - MIN_SIDE)
        if step < 2:
            r = model({k: v.clone() for k, v in data.items()})
            r["loss"].backward()
            opt.step()
            model.zero_grad()
    print(f"{name}: seed {seed}: margins at init / adam1 / adam2 = " + " / ".join(seen))
    return ok


if __name__ == "__main__":
    seed = 1234
    while not all(recorded_states_ok(name, seed) for name in CASES):
        seed += 1
    print(f"mtl: model seed {seed}")
    for name, (_, _, train_mode) in CASES.items():
        G.dump_model_case(name, lambda: build(name), seed=seed, train_mode=train_mode)
        g = dict(np.load(os.path.join(HERE, f"model_{name}.npz")))
        params = [k[5:] for k in g if k.startswith("init/")]
        assert sorted(k[5:] for k in g if k.startswith("grad/")) == sorted(params), f"{name}: a parameter has no gradient"
        shape = (G.B, 1) if name.startswith("essm") else (G.B,)
        assert g["out/task1_pred"].shape == shape and g["out/task2_pred"].shape == shape, name
