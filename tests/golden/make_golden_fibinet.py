#!/usr/bin/env python
"""FiBiNet / AFM golden vectors, produced by RUNNING the upstream reference (build container only):

    PYTHONHASHSEED=0 python tests/golden/make_golden_fibinet.py

  model_fibinet.npz    rec_pangu/models/ranking/fibinet.py:13-77 (FiBiNet) with layers/interaction.py:55-81
                       (BilinearInteractionLayer, 'field_interaction') and :238-251 (SENET_Layer), embedding_dim=8, on
                       make_golden.py's small schema and batch (5 sparse + 3 dense features: 10 pairs, one SENET unit).
                       Groups init/ batch/ out/ grad/ adam2/ adam2_out/ as make_golden.dump_model_case writes them.
                       The reference's AFM (ranking/afm.py:14-68, "Fixme: change the current code of AFM with the right
                       version") builds the same layers in the same order: the generator builds it with the same seed and
                       ASSERTS that its init, outputs, gradients, Adam states and inference outputs equal FiBiNet's bit for
                       bit, so the one fixture serves both names.
  fibinet_layers.npz   senet/: SENET_Layer(5, 3) — W1, W2, an input x [6, 5, 8], the output, a cotangent and the gradients of
                       x, W1, W2 under it; <type>/ for BilinearInteractionLayer(5, 8, type), type in field_all / field_each /
                       field_interaction: w<k> (the matrices in module order), x, out [6, 10, 8], cot, dx and dw<k> (field_each:
                       the last field opens no pair, its matrix has no gradient and no dw entry).

Seed choice.  The SENET's two ReLUs are kinks: where a pre-activation is closer to 0 than two fp32 implementations' rounding
difference, they may disagree about the unit being active.  The generator evaluates the pre-activations in float64 at the
three states the model fixture records (the initial weights, after the first and after the second Adam step) and takes the
FIRST model seed from 1234 upward at which every one of them is at least 1e-5 in magnitude (or exactly 0 as a sum over an
all-zero hidden layer, which every implementation reproduces).  It prints the seed; the tests
build their models with it (tests/test_fibinet_host.py: SEED).
Only data is written: no reference source, bytecode or pickled reference objects.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (installs the import shim; its generators only run under __main__)

from rec_pangu.models.ranking import FiBiNet, AFM  # noqa: E402
from rec_pangu.models.layers import SENET_Layer, BilinearInteractionLayer  # noqa: E402

MARGIN = 1e-5
KW = dict(embedding_dim=8)


def senet_margin(Z, W1, W2):
    """the smallest |pre-activation| of a SENET over the field means Z, in float64.  A sample whose hidden units are all
    inactive has second pre-activations that are sums over zeros — exactly 0 in every implementation, so not a kink that
    rounding can cross — and they are left out."""
    pre1 = Z.double() @ W1.double().t()
    hidden = torch.relu(pre1)
    pre2 = (hidden @ W2.double().t())[(hidden > 0).any(dim=1)]
    return min(float(pre1.abs().min()), float(pre2.abs().min()) if pre2.numel() else float("inf"))


def min_margin(model, data):
    with torch.no_grad():
        return senet_margin(model.embedding_layer(data).mean(dim=-1), model.senet_layer.excitation[0].weight,
                            model.senet_layer.excitation[2].weight)


def margins_of_the_recorded_states(seed):
    torch.manual_seed(seed)
    model = FiBiNet(enc_dict=G.small_enc_dict(), **KW)
    model.train(False)
    data = G.small_batch()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    out = [min_margin(model, data)]
    for _ in range(2):
        r = model({k: v.clone() for k, v in data.items()})
        r["loss"].backward()
        opt.step()
        model.zero_grad()
        out.append(min_margin(model, data))
    return out


def make_layers():
    out = {}
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(21)
    layer = SENET_Layer(5, 3)
    x = torch.randn(6, 5, 8, generator=g).requires_grad_(True)
    cot = torch.randn(6, 5, 8, generator=g)
    y = layer(x)
    y.backward(cot)
    with torch.no_grad():
        assert senet_margin(x.mean(-1), layer.excitation[0].weight, layer.excitation[2].weight) >= MARGIN
    out.update({"senet/W1": G.to_np(layer.excitation[0].weight), "senet/W2": G.to_np(layer.excitation[2].weight),
                "senet/x": G.to_np(x), "senet/out": G.to_np(y), "senet/cot": G.to_np(cot), "senet/dx": G.to_np(x.grad),
                "senet/dW1": G.to_np(layer.excitation[0].weight.grad), "senet/dW2": G.to_np(layer.excitation[2].weight.grad)})
    for t in ("field_all", "field_each", "field_interaction"):
        torch.manual_seed(22)
        layer = BilinearInteractionLayer(5, 8, t)
        mods = [layer.bilinear_layer] if t == "field_all" else list(layer.bilinear_layer)
        x = torch.randn(6, 5, 8, generator=g).requires_grad_(True)
        cot = torch.randn(6, 10, 8, generator=g)
        y = layer(x)
        y.backward(cot)
        out.update({f"{t}/x": G.to_np(x), f"{t}/out": G.to_np(y), f"{t}/cot": G.to_np(cot), f"{t}/dx": G.to_np(x.grad)})
        for k, m in enumerate(mods):
            out[f"{t}/w{k}"] = G.to_np(m.weight)
            if m.weight.grad is not None:
                out[f"{t}/dw{k}"] = G.to_np(m.weight.grad)
    np.savez_compressed(os.path.join(HERE, "fibinet_layers.npz"), **out)
    print("wrote fibinet_layers", len(out), "arrays")


if __name__ == "__main__":
    seed = 1234
    while True:
        margins = margins_of_the_recorded_states(seed)
        print(f"fibinet: seed {seed}: SENET margins at init / adam1 / adam2 = " + " / ".join(f"{m:.3g}" for m in margins))
        if min(margins) >= MARGIN:
            break
        seed += 1
    print(f"fibinet: model seed {seed}")
    G.dump_model_case("fibinet", lambda: FiBiNet(enc_dict=G.small_enc_dict(), **KW), seed=seed, train_mode=False)
    fib = dict(np.load(os.path.join(HERE, "model_fibinet.npz")))
    G.dump_model_case("afm_check", lambda: AFM(enc_dict=G.small_enc_dict(), **KW), seed=seed, train_mode=False)
    path = os.path.join(HERE, "model_afm_check.npz")
    afm = dict(np.load(path))
    os.remove(path)
    assert list(afm) == list(fib), "AFM's arrays differ from FiBiNet's in name or order"
    for k in fib:
        assert afm[k].shape == fib[k].shape and afm[k].tobytes() == fib[k].tobytes(), f"AFM differs from FiBiNet at {k}"
    print("AFM == FiBiNet bit for bit over", len(fib), "arrays: model_fibinet.npz serves both names")
    make_layers()
