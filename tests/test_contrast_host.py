"""CLRec, ContraRec, the BERT4RecEncoder and the in-batch contrastive loss on the CPU (plumbing, no GPU): the host statement
of the loss against float64 transcriptions of the reference's two losses, the three models against the golden files produced
by running the reference (tests/golden/make_golden_contrast.py) with the recorded augmentations replayed through
data_augmenter.augment, the encoder's state_dict order, the encoder names, and the vectorised DataAugmenter's structure.

Bars of the model comparisons are tests/test_sequence_host.py's: out 1e-5, everything else 1e-4, the other tolerance 1e-6,
the tighter of the two readings per element (the generator chose its seeds against a tenth of that).

adam2/ leaves out what Adam turns from rounding noise into lr-sized steps (make_golden_contrast.py has the reasoning): the key
biases, whose gradient is exactly zero, and, in ContraRec-GRU's file only, the 12 of 153384 entries the generator marked in
adam2_skip/ because the reference's own fp32 and float64 runs disagree there by more than a tenth of the bar.  Those are held
to what Adam guarantees instead, |adam2 - init| <= 2.1 lr (tests/test_sasrec_host.py derives
it); `grad/` holds every entry to the bar and adam2_out/ is compared in full."""
import os

import pytest
import torch

from conftest import GOLDEN, load_golden
from test_sequence_host import close

torch.set_num_threads(1)

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
CASES = {"clrec": ("CLRec", {}), "contrarec_bert": ("ContraRec", {}), "contrarec_gru": ("ContraRec", {"encoder_name": "GRU4Rec"})}
KEY_BIAS = "k_linear.bias"
LR = 1e-2


def golden(case):
    """model_<case>.npz, with the groups the generator had to put into files of their own"""
    g = load_golden(f"model_{case}.npz")
    for suffix in ("_grad", "_adam2"):
        if os.path.exists(os.path.join(GOLDEN, f"model_{case}{suffix}.npz")):
            g.update(load_golden(f"model_{case}{suffix}.npz"))
    return g


def build(case, seed):
    from rec_pangu_amd.models import sequence
    name, cfg = CASES[case]
    torch.manual_seed(seed)
    return getattr(sequence, name)(ENC, dict(CONFIG, **cfg)).train()


class Replay:
    """stands in for data_augmenter.augment: hands out the recorded results in call order"""

    def __init__(self, items, device):
        self.items, self.device, self.n = items, device, 0

    def __call__(self, seqs):
        out = self.items[self.n].to(self.device)
        self.n += 1
        assert out.shape == seqs.shape
        return out


def replay(model, g, first, device):
    if hasattr(model, "data_augmenter"):
        model.data_augmenter.augment = Replay([g["aug"][str(i)] for i in range(first, len(g["aug"]))], device)


def run_case(case, g, device="cpu", make_opt=None):
    """(out, grads, adam2, adam2_out) of our model on `device`, as the generator runs the reference (shared with
    tests/test_hip_contrast_models.py)"""
    seed = int(g["seed"])
    batch = {k: v.to(device) for k, v in g["batch"].items()}
    model = build(case, seed).to(device)
    replay(model, g, 0, device)
    res = model({k: v.clone() for k, v in batch.items()})
    model.zero_grad()
    res["loss"].backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    model = build(case, seed).to(device)
    replay(model, g, 2, device)
    opt = (make_opt(model) if make_opt is not None
           else torch.optim.Adam(model.parameters(), lr=LR, betas=(0.9, 0.999), eps=1e-08, weight_decay=0))
    for _ in range(2):
        model({k: v.clone() for k, v in batch.items()})["loss"].backward()
        opt.step()
        model.zero_grad()
    adam2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        r = model({k: v.clone() for k, v in batch.items()}, is_training=False)
    return out, grads, adam2, {k: v.detach().cpu() for k, v in r.items()}


def check_against_golden(g, out, grads, adam2, adam2_out, closer=close):
    """shared with tests/test_hip_contrast_models.py, which passes what the HIP path computed"""
    assert set(g["out"]) == {"loss"} and "user_emb" in out  # (the reference returns the loss alone while training)
    closer("out", out["loss"], g["out"]["loss"], "out loss")
    assert set(grads) == set(g["grad"])
    for k, v in g["grad"].items():
        closer("grad", grads[k], v, f"grad {k}")
    assert list(adam2) == list(g["adam2"])
    skip = g.get("adam2_skip", {})
    for k, v in g["adam2"].items():
        if k.endswith(KEY_BIAS):
            noise = torch.ones_like(v, dtype=torch.bool)
        else:
            noise = skip[k].bool() if k in skip else torch.zeros_like(v, dtype=torch.bool)
        init = g["init"][k]
        for t in (adam2[k], v):  # (the reference's own noise obeys the same bound)
            assert float(((t - init).abs() * noise).max()) <= 2.1 * LR, k
        closer("adam2", torch.where(noise, v, adam2[k]), v, f"adam2 {k}")
    assert set(adam2_out) == set(g["adam2_out"]) == {"user_emb"}
    closer("adam2_out", adam2_out["user_emb"], g["adam2_out"]["user_emb"], "adam2_out user_emb")


@pytest.mark.parametrize("case", list(CASES))
def test_model_against_the_reference_golden(case):
    g = golden(case)
    model = build(case, int(g["seed"]))
    assert list(model.state_dict()) == list(g["init"])  # names and registration order
    for k, v in model.state_dict().items():
        assert torch.equal(v, g["init"][k]), k  # the init RNG stream
    assert (len(g.get("aug", {})) == 6) == (case != "clrec")
    marked = sum(int(v.sum()) for v in g.get("adam2_skip", {}).values())
    assert marked == (12 if case == "contrarec_gru" else 0)
    check_against_golden(g, *run_case(case, g))


def test_encoder_parameter_names_and_order():
    from rec_pangu_amd.models.layers import BERT4RecEncoder
    from rec_pangu_amd.models.layers import sequence as seq_layers
    g = golden("clrec")
    enc = BERT4RecEncoder(D, L, num_layers=2, num_heads=2)
    want = [k[len("encoder."):] for k in g["init"] if k.startswith("encoder.")]
    assert list(enc.state_dict()) == want and want[0] == "p_embeddings.weight"
    block = [f"masked_attn_head.{m}.{p}" for m in ("q_linear", "k_linear", "v_linear") for p in ("weight", "bias")] + \
        [f"{m}.{p}" for m in ("layer_norm1", "linear1", "linear2", "layer_norm2") for p in ("weight", "bias")]
    assert want[1:] == [f"transformer_block.{i}.{k}" for i in range(2) for k in block]
    assert enc.p_embeddings.weight.shape == (L + 1, D) and enc.transformer_block[0].layer_norm1.eps == 1e-5
    assert enc.transformer_block[0].dropout1.p == 0 and enc.transformer_block[0].linear1.out_features == D
    same = seq_layers.MultiHeadAttention(8, 2, kq_same=True)
    assert list(same.state_dict()) == ["k_linear.weight", "k_linear.bias", "v_linear.weight", "v_linear.bias"]


def test_encoder_names():
    from rec_pangu_amd.models.sequence import ContraRec
    with pytest.raises(NotImplementedError, match="Caser"):
        ContraRec(ENC, dict(CONFIG, encoder_name="Caser"))
    with pytest.raises(ValueError):
        ContraRec(ENC, dict(CONFIG, encoder_name="LSTM"))
    m = ContraRec(ENC, dict(CONFIG))
    assert (m.gamma, m.beta_a, m.beta_b, m.ctc_temp, m.ccc_temp, m.encoder_name) == (1, 3, 3, 0.2, 0.2, "BERT4Rec")
    assert m.data_augmenter.num_items == V - 1
    from rec_pangu_amd.models.sequence import CLRec
    assert CLRec(ENC, dict(CONFIG)).temp == 0.1 and CLRec(ENC, dict(CONFIG, temp=0.3)).temp == 0.3


def test_an_empty_row_gives_a_zero_vector_and_finite_gradients():
    from rec_pangu_amd.models.layers import BERT4RecEncoder
    torch.manual_seed(3)
    enc = BERT4RecEncoder(D, L)
    seq = torch.randn(3, L, D, requires_grad=True)
    out = enc(seq, torch.tensor([2, 0, L]))
    assert float(out[1].detach().abs().max()) == 0.0 and float(out[0].detach().abs().max()) > 0
    out.sum().backward()
    assert bool(torch.isfinite(seq.grad).all()) and float(seq.grad[1].abs().max()) == 0.0
    assert all(bool(torch.isfinite(p.grad).all()) for p in enc.parameters())


# ---- the loss: the host statement against float64 transcriptions of the reference's two modules ------------------------------
def clrec_loss_f64(user, item, temperature):
    """clrec.py:65-102 at its default mask (the identity): every user row against every target row, its own the positive"""
    dot = user.double() @ item.double().T / temperature
    logits = dot - dot.max(dim=1, keepdim=True).values
    log_prob = logits - torch.log(torch.exp(logits).sum(1, keepdim=True) + 1e-10)
    return -torch.diagonal(log_prob).mean()


def contrarec_loss_f64(view1, view2, labels, temperature):
    """contrarec.py:93-144: the 2 B views against each other, positives by equal label, the view itself left out of both the
    positives and the denominator, the mean log-likelihood of the positives times -temperature"""
    f = torch.cat([view1, view2], dim=0).double()
    lab = torch.cat([labels, labels])
    n = f.shape[0]
    dot = f @ f.T / temperature
    logits = dot - dot.max(dim=1, keepdim=True).values
    others = ~torch.eye(n, dtype=torch.bool)
    positives = ((lab[:, None] == lab[None, :]) & others).double()
    log_prob = logits - torch.log((torch.exp(logits) * others).sum(1, keepdim=True) + 1e-10)
    return (-temperature * (positives * log_prob).sum(1) / (positives.sum(1) + 1e-10)).mean()


@pytest.mark.parametrize("B,d,T", [(2, 12, 0.2), (5, 8, 0.1), (33, 64, 0.05), (64, 128, 0.2)])
def test_the_host_statement_is_the_reference_s_two_losses(B, d, T):
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(B * 100 + d)
    u, v = (torch.nn.functional.normalize(torch.randn(B, d, generator=gen), dim=-1) for _ in range(2))
    own = torch.arange(B)
    labels = torch.randint(0, 4, (B,), generator=gen)
    for fn in (Fh.contrastive_loss_reference, Fh.contrastive_loss):  # (on CPU tensors the public function is the statement)
        ref = clrec_loss_f64(u, v, T)
        # (CLRec's module does not divide by the number of positives, 1 there; the one formula divides by 1 + 1e-10)
        assert abs(float(fn(u.double(), v.double(), own, own, T)) - float(ref)) <= 2e-10 * max(1.0, abs(float(ref)))
        assert abs(float(fn(u, v, own, own, T)) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
        ref = contrarec_loss_f64(u, v, labels, T)
        f, lab = torch.cat([u, v]), torch.cat([labels, labels])
        assert abs(float(fn(f.double(), None, lab, None, T, True, T)) - float(ref)) <= 1e-12 * max(1.0, abs(float(ref)))
        assert abs(float(fn(f, None, lab, None, T, True, T)) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref)))
    with pytest.raises(ValueError):
        Fh.contrastive_loss(u, v, own, own, T, exclude_self=True)
    with pytest.raises(ValueError):
        Fh.contrastive_loss(u, None, own, own, T)
    with pytest.raises(ValueError):
        Fh.contrastive_loss(u, v, own, own, 0.0)


def test_a_row_without_positives_adds_nothing():
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(4, 6, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(3, 6, generator=gen, dtype=torch.float64)
    la, lb = torch.tensor([0, 9, 1, 0]), torch.tensor([0, 1, 0])
    loss = Fh.contrastive_loss(a, b, la, lb, 0.5)
    loss.backward()
    assert float(a.grad[1].abs().max()) == 0.0 and float(a.grad[0].abs().max()) > 0
    keep = torch.tensor([0, 2, 3])
    assert abs(float(loss.detach()) - float(Fh.contrastive_loss(a.detach()[keep], b, la[keep], lb, 0.5)) * 3 / 4) <= 1e-12


def test_the_new_entry_points_are_declared_and_bound():
    from rec_pangu_amd import hip
    for name in ("rp_contrast_fits", "rp_contrast_geometry", "rp_contrast_workspace_bytes", "rp_contrast_fwd", "rp_contrast_bwd",
                 "rp_seq_attn_keypad_fwd", "rp_seq_attn_keypad_bwd"):
        assert name in hip.EXPORTED_SYMBOLS, name
    for fn in ("contrast_fwd", "contrast_bwd", "contrast_fits", "contrast_geometry", "contrast_workspace_bytes"):
        assert callable(getattr(hip, fn))


# ---- the vectorised augmenter ---------------------------------------------------------------------------------------------
def check_augmenter(device):
    """the structure of DataAugmenter.augment from its returned plan (shared with tests/test_hip_contrast_models.py)"""
    from rec_pangu_amd.models.sequence.contrarec import DataAugmenter
    B, Ls, num_items = 2000, 20, 99
    gen = torch.Generator().manual_seed(7)
    seqs = torch.randint(1, num_items, (B, Ls), generator=gen)
    seqs[:, 15:] = 0  # pads are augmented like content, as in the reference
    seqs = seqs.to(device)
    aug = DataAugmenter(beta_a=3, beta_b=3, num_items=num_items)
    torch.manual_seed(11)
    out, (is_mask, count, start) = aug.augment(seqs, return_plan=True)
    torch.manual_seed(11)
    again = aug.augment(seqs)
    assert torch.equal(out, again) and out.device == seqs.device and out.dtype == seqs.dtype and out.shape == seqs.shape
    assert not torch.equal(out, aug.augment(seqs))  # (the stream moves on)
    out, is_mask, count, start, seqs = (t.cpu() for t in (out, is_mask, count, start, seqs))
    assert is_mask.dtype == torch.bool and 0.3 * B < int(is_mask.sum()) < 0.7 * B  # both kinds occur (a fair coin: 20 sigma)
    assert int(count.min()) >= 0 and int(count.max()) <= Ls and int(start.min()) >= 0 and bool((start <= Ls - count).all())
    assert 0.4 * Ls < float(count.double().mean()) < 0.55 * Ls  # Beta(3, 3): mean 1/2, int() rounds down
    changed = out != seqs
    m = is_mask
    assert bool((changed[m].sum(1) <= count[m]).all())  # (a chosen position that already holds num_items cannot show)
    assert bool((out[m][changed[m]] == num_items).all())
    assert int((changed[m].sum(1) == count[m]).sum()) == int(m.sum())  # ids lie in [1, num_items): every chosen position shows
    pos = torch.arange(Ls)[None, :]
    inside = (pos >= start[:, None]) & (pos < (start + count)[:, None])
    r = ~is_mask
    assert not bool((changed & ~inside)[r].any())
    big = Ls + num_items + 1  # sorts the outside positions out of the way
    a = torch.where(inside, seqs, torch.full_like(seqs, big)).sort(dim=1).values
    b = torch.where(inside, out, torch.full_like(out, big)).sort(dim=1).values
    assert torch.equal(a[r], b[r])  # the same multiset inside the window
    assert int((changed[r].sum(1) > 0).sum()) > 0.5 * int(r.sum())  # (and the windows are permuted)


def test_the_augmenter_s_structure():
    check_augmenter("cpu")
