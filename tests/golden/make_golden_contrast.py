#!/usr/bin/env python
"""CLRec and ContraRec golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_contrast.py

  model_clrec.npz            rec_pangu/models/sequence/clrec.py, the defaults (temp 0.1; BERT4RecEncoder, 2 layers, 2 heads)
  model_contrarec_bert.npz   rec_pangu/models/sequence/contrarec.py, the defaults (gamma 1, beta 3 / 3, ccc_temp 0.2, 'BERT4Rec')
  model_contrarec_gru.npz    the same with encoder_name 'GRU4Rec' (GRU4RecEncoder, hidden 128); its 153384 parameters make
                             three groups of 0.6 MB each, more than one committed file may hold, so grad/ lies in
                             model_contrarec_gru_grad.npz and adam2/ with adam2_skip/ in model_contrarec_gru_adam2.npz

The layout, the batch (V = 37, D = 8, L = 6, B = 5, a repeated target) and the seed discipline are make_golden_sasrec.py's:
groups init/ batch/ out/ grad/ adam2/ adam2_out/, two Adam steps at lr = 1e-2; per file the model seed is the FIRST from 1234
upward at which the reference in fp32 and a float64 copy of it, stepped side by side, agree within a TENTH of the bars of
tests/test_contrast_host.py (out 1e-5, everything else 1e-4, 1e-6 as the other tolerance).  The key biases (`k_linear.bias`)
stay out of adam2 for make_golden_sasrec.py's reason: their gradient is exactly zero, Adam turns its rounding noise into
lr-sized steps.  ContraRec's GRU encoder (hidden 128: 49152 recurrent weights per layer over a batch of 5) shows the same
effect in single entries: Adam's second step depends on the RATIO of two gradients, the reference's fp32 gradient differs from
its float64 copy's by up to 2e-7 absolutely, and among 153384 entries some have a gradient small enough for that to move them
by more than the bar, at every one of 2000 seeds.  In that file alone adam2_skip/<key> (uint8) marks exactly the entries in
which the reference's own fp32 and float64 runs disagree by more than a tenth of the bar after the two steps; the tests
leave them out of adam2 and bound their distance from init/ by Adam's step instead.  The other two files mark nothing.
adam2_out is compared in full.

ContraRec draws its augmentations at random: every result of data_augmenter.augment() is recorded, in call order, under
aug/<n> (two for the out/ and grad/ run, then two per Adam step), and the tests replay them through the same method.  In the
seed search the float64 copy replays the fp32 model's augmentations.

Every attention of the golden runs is checked for the one place where the port's formula differs from the reference's (it
subtracts each row's own maximum score, the reference the maximum of the whole batch tensor): the batch maximum exceeds no
row's maximum by more than 20, asserted below, so exp() is nowhere near underflow and the two agree to rounding.

Printed by the run that wrote the committed fixtures (the first and the accepted line of each file; every seed between
them was rejected in the same way, 266 lines in all; 12 of the GRU file's 153384 entries are marked):

  clrec: seed 1234: fp32-f64 over bar/10: out 0.074 grad 1.5 adam2 0.59 adam2_out 1.4 | rejected
  clrec: seed 1471: fp32-f64 over bar/10: out 0.18 grad 0.89 adam2 0.3 adam2_out 0.79 | ok
  contrarec_bert: seed 1234: fp32-f64 over bar/10: out 0.013 grad 1.3 adam2 0.63 adam2_out 0.62 | rejected
  contrarec_bert: seed 1247: fp32-f64 over bar/10: out 0.27 grad 0.82 adam2 0.9 adam2_out 0.85 | ok
  contrarec_gru: seed 1234: fp32-f64 over bar/10: out 0.26 grad 0.62 adam2 1 adam2_out 35 | rejected
  contrarec_gru: seed 1247: fp32-f64 over bar/10: out 0.14 grad 0.8 adam2 0.99 adam2_out 0.48 | ok
  largest gap between the batch maximum and a row's own maximum score: 17.6

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

from rec_pangu.models.layers import sequence as ref_sequence  # noqa: E402
from rec_pangu.models.sequence import CLRec, ContraRec  # noqa: E402
from make_golden_sasrec import BARS, CONFIG, ENC, adam, batch, to_np  # noqa: E402

KEY_BIAS = "k_linear.bias"
MARK = ("contrarec_gru",)  # files that mark the entries in which the reference's fp32 and float64 runs disagree after Adam
SPLIT = ("contrarec_gru",)  # files whose groups do not fit one committed file
CASES = {
    "clrec": dict(cls=CLRec, config={}),
    "contrarec_bert": dict(cls=ContraRec, config={}),
    "contrarec_gru": dict(cls=ContraRec, config={"encoder_name": "GRU4Rec"}),
}
MAX_GAP = {"seen": 0.0}

_attention = ref_sequence.MultiHeadAttention.scaled_dot_product_attention


def checked_attention(q, k, v, d_k, mask=None):
    scores = torch.matmul(q, k.transpose(-2, -1)) / d_k ** 0.5
    if mask is not None:
        scores = scores.masked_fill(mask == 0, -np.inf)
    gap = float((scores.detach().max() - scores.detach().max(dim=-1).values).max())
    assert gap <= 20.0, f"the batch maximum lies {gap} above a row's own maximum"
    MAX_GAP["seen"] = max(MAX_GAP["seen"], gap)
    return _attention(q, k, v, d_k, mask)


ref_sequence.MultiHeadAttention.scaled_dot_product_attention = staticmethod(checked_attention)


class Tape:
    """records every result of augment(), or replays a recorded list"""

    def __init__(self, augmenter, replay=None):
        self.inner, self.items, self.replay = augmenter.augment, [], replay

    def __call__(self, seqs):
        out = self.inner(seqs) if self.replay is None else self.replay[len(self.items)].clone()
        self.items.append(out.clone())
        return out


def build(case):
    return case["cls"](ENC, dict(CONFIG, **case["config"])).train()


def tape(model, replay=None):
    if not hasattr(model, "data_augmenter"):
        return None
    t = Tape(model.data_augmenter, replay)
    model.data_augmenter.augment = t
    return t


def worst(group, got, want, skip=None):
    """largest |fp32 - f64| over a tenth of the bar; the bar is the tighter of (atol, rtol) = (big, 1e-6) and (1e-6, big)"""
    big, small = BARS[group]
    w = 0.0
    for k, v in want.items():
        if group == "adam2" and k.endswith(KEY_BIAS):
            continue
        v = v.detach()
        bar = torch.minimum(big + small * v.abs(), small + big * v.abs())
        over = (got[k].detach().double() - v).abs() / (bar / 10)
        if skip is not None and k in skip:
            over = over.masked_fill(skip[k], 0.0)
        w = max(w, float(over.max()))
    return w


def check(name, case, seed):
    torch.manual_seed(seed)
    m32 = build(case)
    m64 = copy.deepcopy(m32).double()
    t32 = tape(m32)
    t64 = tape(m64, replay=t32.items if t32 is not None else None)
    opts = [adam(m32), adam(m64)]
    data = batch()
    agree, skip = {}, {}
    for step in range(3):
        if step == 2:
            with torch.no_grad():
                agree["adam2_out"] = worst("adam2_out", m32(data, is_training=False), m64(data, is_training=False))
            break
        r32 = m32(data)
        r64 = m64(data)
        r32["loss"].backward(), r64["loss"].backward()
        if step == 0:
            agree["out"] = worst("out", r32, r64)
            agree["grad"] = worst("grad", {k: p.grad for k, p in m32.named_parameters()},
                                  {k: p.grad for k, p in m64.named_parameters()})
        for o, m in zip(opts, (m32, m64)):
            o.step()
            m.zero_grad()
        if step == 1:
            if name in MARK:
                big, small = BARS["adam2"]
                for (k, a), b in zip(m32.state_dict().items(), m64.state_dict().values()):
                    bar = torch.minimum(big + small * b.abs(), small + big * b.abs())
                    skip[k] = (a.double() - b).abs() > bar / 10
            agree["adam2"] = worst("adam2", m32.state_dict(), m64.state_dict(), skip)
    assert t64 is None or len(t64.items) == len(t32.items) == 4
    ok = max(agree.values()) <= 1.0
    print(f"  {name}: seed {seed}: fp32-f64 over bar/10: " + " ".join(f"{k} {v:.2g}" for k, v in agree.items()) +
          (" | ok" if ok else " | rejected"))
    return skip if ok else None


def dump_model(name, case, seed, skip):
    out = {"seed": np.asarray(seed)}
    for k, v in skip.items():
        if bool(v.any()) and not k.endswith(KEY_BIAS):
            out["adam2_skip/" + k] = to_np(v.to(torch.uint8))
    skipped = sum(int(v.sum()) for v in skip.values()), sum(p.numel() for p in build(case).parameters())
    data = batch()
    augs = []
    torch.manual_seed(seed)
    model = build(case)
    t = tape(model)
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
    if t is not None:
        augs += t.items
    torch.manual_seed(seed)
    model = build(case)
    t = tape(model)
    opt = adam(model)
    for _ in range(2):
        model(data)["loss"].backward()
        opt.step()
        model.zero_grad()
    if t is not None:
        augs += t.items
    for i, a in enumerate(augs):
        out[f"aug/{i}"] = to_np(a)
    for k, v in model.state_dict().items():
        out["adam2/" + k] = to_np(v)
    with torch.no_grad():
        for k, v in model(data, is_training=False).items():
            out["adam2_out/" + k] = to_np(v)
    files = {"": out}
    if name in SPLIT:
        files = {"_grad": {k: v for k, v in out.items() if k.startswith("grad/")},
                 "_adam2": {k: v for k, v in out.items() if k.startswith(("adam2/", "adam2_skip/"))}}
        files[""] = {k: v for k, v in out.items() if k not in files["_grad"] and k not in files["_adam2"]}
    for suffix, arrays in files.items():
        path = os.path.join(HERE, f"model_{name}{suffix}.npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < 1 << 20, path
    print(f"wrote model_{name}.npz", len(out), "arrays,", len(augs), "augmentations,", skipped[0], "of", skipped[1],
          "entries left out of adam2")


if __name__ == "__main__":
    for name, case in CASES.items():
        seed = 1234
        skip = check(name, case, seed)
        while skip is None:
            seed += 1
            assert seed < 1234 + 2000, "no seed found"
            skip = check(name, case, seed)
        dump_model(name, case, seed, skip)
    print(f"  largest gap between the batch maximum and a row's own maximum score: {MAX_GAP['seen']:.3g}")
