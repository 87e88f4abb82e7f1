#!/usr/bin/env python
"""AFN golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_afn.py

  model_afn_eval.npz        rec_pangu/models/ranking/afn.py:14-102, embedding_dim=8, dnn_hidden_units = afn_hidden_units = [8, 4],
                            logarithmic_neurons=3, ensemble_dnn=True, unmodified (both MLPs keep the default dropout of 0.1),
                            eval mode: both BatchNorms on their running statistics, dropout inactive
  model_afn_train.npz       the same in train mode (batch statistics, running buffers move) with every nn.Dropout.p set to 0
  model_afn_noens_eval.npz  ensemble_dnn=False (no embedding_layer2 / dnn / fc), eval mode
on make_golden.py's small schema and batch (5 sparse features, B = 24).  Groups init/ batch/ out/ grad/ after1/ adam2/
adam2_out/ as make_golden.dump_model_case writes them.

Seed choice.  Three things make a correct fp32 implementation disagree with another one here, so the generator takes, for each
case on its own, the FIRST model seed from 1234 upward at which, at the three states a fixture records (the forward at the
initial weights, the forward after the first Adam step, the inference forward after the second), all of these hold:
  * every ReLU pre-activation (float64 copy) is at least 1e-5 from 0;
  * every looked-up |e| of embedding_layer is at least 1e-7 from the clamp threshold float32(1e-5);
  * every prediction lies in [1e-3, 1 - 1e-3] (eval mode at init feeds an unnormalised log|e| into exp: it often saturates);
  * the reference in fp32 and a float64 copy of it, stepped side by side, agree within a TENTH of the bar the tests use
    (tests/test_afn_host.py) on every quantity the tests compare: out, grad, after1, adam2 and adam2_out.
In train mode log_batch_norm.bias has no real gradient (a shift of y_f scales c_l by a constant, which exp_batch_norm's batch
statistics remove): the reference's own gradient there is fp32 noise, and Adam turns noise into steps of up to lr.  As in the
tests, that gradient is judged against the bar of log_batch_norm.weight's gradient, the parameter is left out of adam2 and
adam2_out is not compared for the train case.  The same shift scales c_l itself, so exp_batch_norm's RUNNING buffers after the
second step carry that noise too (the reference in fp32 against itself in float64: up to 1e-3 relative at most seeds); they
are pinned by after1/ (before any Adam step) and left out of adam2 for the train case as well.

It prints the seeds and the margins; the tests build their models with them (tests/test_afn_host.py: SEEDS).
Printed by the run that wrote the committed fixtures:

  afn_eval: seed 1245: relu 0.0065/0.002/0.004 | thr 0.0038/0.0026/0.0031 | min(p,1-p) 0.082/0.1/0.087 | fp32-f64 over
            bar/10: out 0.22 grad 0.15 after1 0 adam2 0.051 adam2_out 0.19 | ok
  afn_train: seed 1236: relu 0.00047/0.00044/0.0041 | thr 0.001/0.00074/0.00058 | min(p,1-p) 0.076/0.21/0.081 | fp32-f64 over
            bar/10: out 0.12 grad 0.094 after1 0.0095 adam2 0.039 | ok
  afn_noens_eval: seed 1238: relu 0.006/0.015/0.015 | thr 0.0018/0.00095/0.00054 | min(p,1-p) 0.39/0.35/0.22 | fp32-f64 over
            bar/10: out 0.14 grad 0.08 after1 0 adam2 0.016 adam2_out 0.15 | ok
  afn: model seeds {'afn_eval': 1245, 'afn_train': 1236, 'afn_noens_eval': 1238}
(relu, thr, min(p, 1 - p): the margins at the three states; the last group: the largest |fp32 - float64| over a tenth of the bar.)
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

from rec_pangu.models.ranking import AFN  # noqa: E402

MARGIN = 1e-5
THR = float(np.float32(1e-5))
THR_MARGIN = 1e-7
P_LO = 1e-3
KW = dict(embedding_dim=8, dnn_hidden_units=[8, 4], afn_hidden_units=[8, 4], logarithmic_neurons=3)
CASES = {  # name -> (ensemble_dnn, train mode)
    "afn_eval": (True, False),
    "afn_train": (True, True),
    "afn_noens_eval": (False, False),
}
# the bars of tests/test_afn_host.py: |got - want| <= atol + rtol |want|
BARS = {"out": (1e-5, 1e-6), "grad": (1e-4, 1e-6), "after1": (1e-4, 1e-6), "adam2": (1e-4, 1e-6), "adam2_out": (1e-5, 1e-6)}
BN1_BIAS = "log_batch_norm.bias"
TRAIN_SKIP = (BN1_BIAS, "exp_batch_norm.running_mean", "exp_batch_norm.running_var")  # of adam2/ in train mode


def build(name):
    ens, train_mode = CASES[name]
    model = AFN(enc_dict=G.small_enc_dict(), ensemble_dnn=ens, **KW)
    if train_mode:
        for m in model.modules():
            if isinstance(m, torch.nn.Dropout):
                m.p = 0.0
    return model


def project_bar(v):
    """tests' _grad_close: 1e-4 max(1e-2, max |ref|)"""
    return 1e-4 * max(1e-2, float(v.abs().max()))


class Probe:
    """margins of one forward of the float64 copy: ReLU pre-activations through hooks, |e| against the threshold"""

    def __init__(self, m64):
        self.pre = []
        self.hooks = [mod.register_forward_hook(lambda _m, inp, _o: self.pre.append(float(inp[0].detach().abs().min())))
                      for mod in m64.modules() if isinstance(mod, torch.nn.ReLU)]

    def take(self):
        out, self.pre = min(self.pre), []
        return out


def worst(group, got, want, skip=(), rel=None):
    """largest |fp32 - f64| / (bar / 10) over the entries of a group"""
    rtol, atol = BARS[group]
    w = 0.0
    for k, v in want.items():
        if k in skip or not v.is_floating_point():
            assert k in skip or torch.equal(got[k], v), k  # (num_batches_tracked)
            continue
        bar = (atol + rtol * v.abs()) if rel is None or k not in rel else torch.full_like(v, rel[k])
        w = max(w, float(((got[k].double() - v).abs() / (bar / 10)).max()))
    return w


def check(name, seed):
    ens, train_mode = CASES[name]
    torch.manual_seed(seed)
    m32 = build(name)
    m32.train(train_mode)
    m64 = copy.deepcopy(m32).double()
    m64.train(train_mode)
    data = G.small_batch()
    d64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in data.items()}
    opts = [torch.optim.Adam(m.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0) for m in (m32, m64)]
    probe = Probe(m64)
    relu, thr, plo, agree = [], [], [], {}
    for step in range(3):
        with torch.no_grad():
            e = m32.embedding_layer(data).abs()
        thr.append(float((e - THR).abs().min()))
        if step == 2:
            m32.eval(), m64.eval()
            with torch.no_grad():
                r32, r64 = m32(dict(data), is_training=False), m64(dict(d64), is_training=False)
            if not train_mode:
                agree["adam2_out"] = worst("adam2_out", r32, r64)
        else:
            r32, r64 = m32(dict(data)), m64(dict(d64))
            r32["loss"].backward(), r64["loss"].backward()
            if step == 0:
                agree["out"] = worst("out", r32, r64)
                g32 = {k: p.grad for k, p in m32.named_parameters()}
                g64 = {k: p.grad for k, p in m64.named_parameters()}
                rel = {BN1_BIAS: project_bar(g64["log_batch_norm.weight"])} if train_mode else None
                agree["grad"] = worst("grad", g32, g64, rel=rel)
                run = lambda m: {k: v for k, v in m.state_dict().items() if "running_" in k}  # noqa: E731
                agree["after1"] = worst("after1", run(m32), run(m64))
            for o, m in zip(opts, (m32, m64)):
                o.step()
                m.zero_grad()
            if step == 1:
                agree["adam2"] = worst("adam2", m32.state_dict(), m64.state_dict(), skip=TRAIN_SKIP if train_mode else ())
        relu.append(probe.take())
        p = torch.cat([r32["pred"].double().flatten(), r64["pred"].flatten()])
        plo.append(float(torch.minimum(p, 1 - p).min()))
    ok = min(relu) >= MARGIN and min(thr) >= THR_MARGIN and min(plo) >= P_LO and max(agree.values()) <= 1.0
    print(f"{name}: seed {seed}: relu " + "/".join(f"{v:.2g}" for v in relu) + " | thr " + "/".join(f"{v:.2g}" for v in thr) +
          " | min(p,1-p) " + "/".join(f"{v:.2g}" for v in plo) + " | fp32-f64 over bar/10: " +
          " ".join(f"{k} {v:.2g}" for k, v in agree.items()) + (" | ok" if ok else " | rejected"))
    return ok


if __name__ == "__main__":
    seeds = {}
    for name in CASES:
        seed = 1234
        while not check(name, seed):
            seed += 1
            assert seed < 1234 + 2000, "no seed found"
        seeds[name] = seed
    print(f"afn: model seeds {seeds}")
    for name, (_, train_mode) in CASES.items():
        G.dump_model_case(name, lambda: build(name), seed=seeds[name], train_mode=train_mode)
        g = dict(np.load(os.path.join(HERE, f"model_{name}.npz")))
        params = [k[5:] for k in g if k.startswith("init/") and "running_" not in k and "num_batches" not in k]
        assert sorted(k[5:] for k in g if k.startswith("grad/")) == sorted(params), f"{name}: a parameter has no gradient"
        assert g["out/pred"].shape == (G.B, 1)
