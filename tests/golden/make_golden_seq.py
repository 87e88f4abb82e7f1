#!/usr/bin/env python
"""Sequence-recall golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_seq.py

  model_yotubednn.npz      rec_pangu/models/sequence/yotubednn.py, item vocabulary V = 37, embedding_dim D = 8, max_length
                           L = 6, a hand-made batch of B = 5: a padded tail (rows 0 and 4), an UNMASKED id 0 (row 1, position
                           1), a fully padded row (2), a repeated target (4 twice) and the targets 0 and V - 1.  Groups
                           init/ batch/ out/ grad/ after1/ adam2/ adam2_out/ as make_golden.dump_model_case writes them
                           (after1/ is empty: the model has no running statistics); two Adam steps at lr = 1e-2.
  sequence_dataset.json    a synthetic frame of 12 users with 6 .. 25 interactions each (user_id, item_id, cate, time), the
                           config, the enc_dict the reference derives, every sample of SequenceDatasetV2 in train / valid /
                           test phase, of SequenceDataset in test phase and in train phase under random.seed(0) (samples
                           taken in index order), and get_test_gd() of both classes (V2: valid and test phase).
  evaluate_recall.json     preds / test_gd / topN cases with the reference's results: a user missing from preds, a user
                           without a hit, repeated hits at different ranks.
  sequence_base_pieces.json  small inputs and results of SequenceBaseModel.gather_indexes and .get_attention_mask.

Seed choice (the discipline of make_golden_afn.py): the model seed is the FIRST from 1234 upward at which the reference in fp32
and a float64 copy of it, stepped side by side, agree within a TENTH of the bars the tests use (tests/test_sequence_host.py:
out 1e-5, everything else 1e-4, with 1e-6 as the other tolerance, BOTH as (atol, rtol) and as (rtol, atol): the tighter of
the two per element) on out, grad, adam2 and adam2_out.  Printed by the run that wrote the committed
fixtures:

  yotubednn: seed 1234: fp32-f64 over bar/10: out 0.095 grad 0.051 adam2 0.0091 adam2_out 0.12 | ok

Only data is written: no reference source, bytecode or pickled reference objects.
"""
import copy
import json
import os
import random
import sys

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402

_ref_import.install()

from rec_pangu.dataset.sequence_dataset import SequenceDataset, SequenceDatasetV2  # noqa: E402
from rec_pangu.models.base_model import SequenceBaseModel  # noqa: E402
from rec_pangu.models.sequence import YotubeDNN  # noqa: E402
from rec_pangu.utils.evaluate import evaluate_recall  # noqa: E402

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
BARS = {"out": (1e-5, 1e-6), "grad": (1e-4, 1e-6), "adam2": (1e-4, 1e-6), "adam2_out": (1e-5, 1e-6)}  # (big, small)


def to_np(t):
    return t.detach().cpu().numpy()


def batch():
    hist = torch.tensor([[3, 7, 7, 12, 0, 0],
                         [5, 0, 9, 36, 1, 2],
                         [0, 0, 0, 0, 0, 0],
                         [36, 35, 34, 33, 32, 31],
                         [7, 0, 0, 0, 0, 0]], dtype=torch.long)
    mask = torch.tensor([[1, 1, 1, 1, 0, 0],
                         [1, 1, 1, 1, 1, 1],
                         [0, 0, 0, 0, 0, 0],
                         [1, 1, 1, 1, 1, 1],
                         [1, 0, 0, 0, 0, 0]], dtype=torch.long)
    target = torch.tensor([[4], [20], [4], [0], [V - 1]], dtype=torch.long)
    return {"hist_item_list": hist, "hist_mask_list": mask, "target_item": target}


def build():
    return YotubeDNN(ENC, dict(CONFIG))


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


def check(seed):
    torch.manual_seed(seed)
    m32 = build()
    m64 = copy.deepcopy(m32).double()
    opts = [adam(m32), adam(m64)]
    agree = {}
    for step in range(3):
        if step == 2:
            m32.eval(), m64.eval()
            with torch.no_grad():
                agree["adam2_out"] = worst("adam2_out", m32(batch(), is_training=False), m64(batch(), is_training=False))
            break
        r32, r64 = m32(batch()), m64(batch())
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
    print(f"yotubednn: seed {seed}: fp32-f64 over bar/10: " + " ".join(f"{k} {v:.2g}" for k, v in agree.items()) +
          (" | ok" if ok else " | rejected"))
    return ok


def dump_model(seed):
    out = {"seed": np.asarray(seed)}
    torch.manual_seed(seed)
    model = build()
    for k, v in model.state_dict().items():
        out["init/" + k] = to_np(v)
    for k, v in batch().items():
        out["batch/" + k] = to_np(v)
    res = model(batch())
    for k, v in res.items():
        out["out/" + k] = to_np(v)
    model.zero_grad()
    res["loss"].backward()
    for k, p in model.named_parameters():
        out["grad/" + k] = to_np(p.grad)
    torch.manual_seed(seed)
    model = build()
    opt = adam(model)
    for _ in range(2):
        model(batch())["loss"].backward()
        opt.step()
        model.zero_grad()
    for k, v in model.state_dict().items():
        out["adam2/" + k] = to_np(v)
    model.eval()
    with torch.no_grad():
        for k, v in model(batch(), is_training=False).items():
            out["adam2_out/" + k] = to_np(v)
    np.savez_compressed(os.path.join(HERE, "model_yotubednn.npz"), **out)
    print("wrote model_yotubednn.npz", len(out), "arrays")


def frame():
    rng = np.random.RandomState(7)
    rows = []
    lengths = [6, 7, 9, 10, 11, 12, 14, 16, 18, 21, 23, 25]
    for u, n in enumerate(lengths):
        items = rng.randint(100, 140, size=n)
        for t, it in enumerate(items):
            rows.append({"user_id": 1000 + u, "item_id": int(it), "cate": f"c{int(it) % 5}", "time": int(rng.randint(0, 5) + 10 * t)})
    order = rng.permutation(len(rows))  # (time_col sorts it back)
    return [rows[i] for i in order]


def plain(sample):
    return {k: (v if isinstance(v, str) else v.tolist()) for k, v in sample.items()}


def dump_dataset():
    rows = frame()
    config = {"max_length": 10, "user_col": "user_id", "item_col": "item_id", "time_col": "time", "cate_cols": ["cate"],
              "next_seq_length": 4}
    out = {"frame": rows, "config": config}

    def make(cls, phase, enc=None):
        return cls(dict(config), pd.DataFrame(rows), enc_dict=enc, phase=phase)

    first = make(SequenceDatasetV2, "train")
    out["enc_dict"] = first.enc_dict
    enc = first.enc_dict
    for phase in ("train", "valid", "test"):
        ds = make(SequenceDatasetV2, phase, enc)
        out[f"v2_{phase}"] = [plain(ds[i]) for i in range(len(ds))]
        if phase != "train":
            out[f"v2_{phase}_gd"] = ds.get_test_gd()
    ds = make(SequenceDataset, "test", enc)
    out["v1_test"] = [plain(ds[i]) for i in range(len(ds))]
    out["v1_test_gd"] = ds.get_test_gd()
    ds = make(SequenceDataset, "train", enc)
    random.seed(0)
    out["v1_train_seed0"] = [plain(ds[i]) for i in range(len(ds))]
    with open(os.path.join(HERE, "sequence_dataset.json"), "w") as f:
        json.dump(out, f, sort_keys=True)
    print("wrote sequence_dataset.json", len(rows), "rows")


def dump_evaluate():
    preds = {"u1": [5, 9, 3, 7, 1, 8], "u2": [2, 4, 6, 8, 10, 12], "u3": [11, 13, 17, 19, 23, 29], "u5": [1, 2, 3, 4, 5, 6]}
    test_gd = {"u1": [3, 5, 40], "u2": [41, 42], "u3": [29], "u4": [1, 2], "u5": [6, 5, 4, 3, 2, 1, 50]}
    cases = []
    for topN in (1, 3, 5, 6, 50):
        cases.append({"topN": topN, "want": evaluate_recall(preds, test_gd, topN)})
    with open(os.path.join(HERE, "evaluate_recall.json"), "w") as f:
        json.dump({"preds": preds, "test_gd": test_gd, "cases": cases}, f, sort_keys=True)
    print("wrote evaluate_recall.json", cases)


def dump_pieces():
    torch.manual_seed(3)
    model = SequenceBaseModel(ENC, dict(CONFIG))
    seq = torch.arange(2 * 4 * 3, dtype=torch.float32).reshape(2, 4, 3) * 0.5 - 2.0
    index = torch.tensor([3, 1])
    mask = torch.tensor([[1.0, 1.0, 1.0, 0.0], [1.0, 0.0, 0.0, 0.0]])
    out = {"gather": {"output": seq.tolist(), "index": index.tolist(), "want": model.gather_indexes(seq, index).tolist()},
           "attention_mask": {"mask": mask.tolist(), "want": model.get_attention_mask(mask).tolist()}}
    with open(os.path.join(HERE, "sequence_base_pieces.json"), "w") as f:
        json.dump(out, f, sort_keys=True)
    print("wrote sequence_base_pieces.json")


if __name__ == "__main__":
    seed = 1234
    while not check(seed):
        seed += 1
        assert seed < 1234 + 2000, "no seed found"
    dump_model(seed)
    dump_dataset()
    dump_evaluate()
    dump_pieces()
