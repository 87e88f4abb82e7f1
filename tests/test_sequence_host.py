"""The sequence-recall family on the CPU (plumbing, no GPU): YotubeDNN against the golden vectors produced by running the
reference (tests/golden/make_golden_seq.py), both datasets and evaluate_recall against their recorded results, the faiss-free
get_recall_predict against a float64 argsort, one SequenceTrainer run, and the declaration / binding / sizing of the new C
entry points.

Bars of the model comparisons: out 1e-5, everything else 1e-4, the other tolerance 1e-6 — asserted BOTH as (atol, rtol) and as
(rtol, atol), i.e. the tighter of the two per element (the generator chose its seed against a tenth of that)."""
import ctypes
import json
import os
import random
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden

torch.set_num_threads(1)

V, D, L = 37, 8, 6
ENC = {"item_id": {"vocab_size": V}}
CONFIG = {"embedding_dim": D, "max_length": L, "device": "cpu", "item_col": "item_id", "cate_cols": []}
BIG = {"out": 1e-5, "grad": 1e-4, "adam2": 1e-4, "adam2_out": 1e-5}


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def build(seed):
    from rec_pangu_amd.models.sequence import YotubeDNN
    torch.manual_seed(seed)
    return YotubeDNN(ENC, dict(CONFIG))


def close(group, got, want, what):
    big = BIG[group]
    torch.testing.assert_close(got, want, rtol=1e-6, atol=big, msg=lambda m: f"{what}: {m}")
    torch.testing.assert_close(got, want, rtol=big, atol=1e-6, msg=lambda m: f"{what}: {m}")


def check_against_golden(g, out, grads, adam2, adam2_out):
    """shared with tests/test_hip_sequence.py, which passes what the HIP path computed"""
    assert set(out) == set(g["out"]) == {"user_emb", "loss"}
    for k, v in g["out"].items():
        close("out", out[k], v, f"out {k}")
    assert set(grads) == set(g["grad"])
    for k, v in g["grad"].items():
        close("grad", grads[k], v, f"grad {k}")
    assert list(adam2) == list(g["adam2"])
    for k, v in g["adam2"].items():
        close("adam2", adam2[k], v, f"adam2 {k}")
    assert set(adam2_out) == set(g["adam2_out"]) == {"user_emb"}
    for k, v in g["adam2_out"].items():
        close("adam2_out", adam2_out[k], v, f"adam2_out {k}")


def run_case(g, device="cpu", make_opt=None):
    """(out, grads, adam2, adam2_out) of our YotubeDNN on `device`, as the generator runs the reference"""
    seed = int(g["seed"])
    batch = {k: v.to(device) for k, v in g["batch"].items()}
    model = build(seed).to(device)
    res = model({k: v.clone() for k, v in batch.items()})
    model.zero_grad()
    res["loss"].backward()
    out = {k: v.detach().cpu() for k, v in res.items()}
    grads = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    model = build(seed).to(device)
    opt = (make_opt(model) if make_opt is not None
           else torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0))
    for _ in range(2):
        model({k: v.clone() for k, v in batch.items()})["loss"].backward()
        opt.step()
        model.zero_grad()
    adam2 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    model.eval()
    with torch.no_grad():
        r = model({k: v.clone() for k, v in batch.items()}, is_training=False)
    return out, grads, adam2, {k: v.detach().cpu() for k, v in r.items()}


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_yotubednn_state_dict_and_init_stream():
    g = load_golden("model_yotubednn.npz")
    model = build(int(g["seed"]))
    sd = model.state_dict()
    assert list(sd) == list(g["init"]) == ["item_emb.weight"]
    assert sd["item_emb.weight"].shape == (V, D)
    assert torch.equal(sd["item_emb.weight"], g["init"]["item_emb.weight"])  # same draws from the same stream
    assert float(sd["item_emb.weight"][0].abs().max()) > 0  # reset_parameters leaves the padding row non-zero
    assert model.item_emb.padding_idx == 0 and isinstance(model.loss_fun, torch.nn.CrossEntropyLoss)


def test_yotubednn_cate_tables_follow_the_item_table():
    from rec_pangu_amd.models.base_model import SequenceBaseModel
    enc = {"item_id": {"vocab_size": 9}, "cate": {"vocab_size": 4}, "brand": {"vocab_size": 5}}
    cfg = dict(CONFIG, cate_cols=["cate", "brand"])
    model = SequenceBaseModel(enc, cfg)
    assert list(model.state_dict()) == ["item_emb.weight", "cate_emb.weight", "brand_emb.weight"]
    assert model.brand_emb.weight.shape == (5, D) and model.max_length == L and model.device == "cpu"


def test_yotubednn_matches_the_reference_on_cpu():
    g = load_golden("model_yotubednn.npz")
    check_against_golden(g, *run_case(g))


def test_the_fixture_batch_holds_its_edge_cases():
    b = load_golden("model_yotubednn.npz")["batch"]
    hist, mask, tgt = b["hist_item_list"], b["hist_mask_list"], b["target_item"].view(-1)
    assert hist.shape == (5, L) and bool(((hist == 0) & (mask == 1)).any())  # an unmasked id 0
    assert bool((mask.sum(1) == 0).any()) and bool(((mask[:, -1] == 0) & (mask[:, 0] == 1)).any())  # padded row, padded tail
    assert len(set(tgt.tolist())) < len(tgt) and 0 in tgt.tolist() and V - 1 in tgt.tolist()


def test_a_batch_of_one_trains():
    """the reference's .squeeze() makes the target 0-d and CrossEntropyLoss raises; .view(-1) here"""
    model = build(1)
    data = {"hist_item_list": torch.tensor([[3, 4, 0, 0, 0, 0]]), "hist_mask_list": torch.tensor([[1, 1, 0, 0, 0, 0]]),
            "target_item": torch.tensor([[5]])}
    res = model(data)
    assert res["user_emb"].shape == (1, D) and res["loss"].dim() == 0
    res["loss"].backward()
    assert torch.isfinite(model.item_emb.weight.grad).all() and float(model.item_emb.weight.grad.abs().max()) > 0


def test_base_model_pieces_against_recorded_values():
    from rec_pangu_amd.models.base_model import SequenceBaseModel
    p = load_json("sequence_base_pieces.json")
    model = SequenceBaseModel(ENC, dict(CONFIG))
    got = model.gather_indexes(torch.tensor(p["gather"]["output"]), torch.tensor(p["gather"]["index"]))
    assert torch.equal(got, torch.tensor(p["gather"]["want"]))
    got = model.get_attention_mask(torch.tensor(p["attention_mask"]["mask"]))
    assert got.shape == (2, 1, 4, 4) and torch.equal(got, torch.tensor(p["attention_mask"]["want"]))
    assert model.output_items() is model.item_emb.weight


def test_functional_cpu_paths_are_the_torch_formulas():
    from rec_pangu_amd import functional as Fh
    gen = torch.Generator().manual_seed(0)
    E = torch.randn(11, 4, generator=gen, requires_grad=True)
    U = torch.randn(3, 4, generator=gen)
    t = torch.tensor([0, 10, 3])
    assert torch.equal(Fh.full_softmax_ce(U, E, t), torch.nn.functional.cross_entropy(U @ E.t(), t))
    hist, mask = torch.tensor([[0, 2, 2], [5, 0, 0]]), torch.tensor([[1, 1, 0], [1, 0, 0]])
    out = Fh.hist_mean(E, hist, mask)
    assert torch.equal(out, (E[hist] * mask[..., None].float()).mean(1))
    out.sum().backward()
    assert float(E.grad[0].abs().max()) == 0 and float(E.grad[2].abs().max()) > 0  # the unmasked id 0 gives row 0 nothing


# ---- datasets -------------------------------------------------------------------------------------------------------------
def _frame(fx):
    import pandas as pd
    return pd.DataFrame(fx["frame"])


def _plain(sample):
    return {k: (v if isinstance(v, str) else v.tolist()) for k, v in sample.items()}


def _check_samples(ds, want):
    assert len(ds) == len(want) == 12
    for i, w in enumerate(want):
        s = ds[i]
        assert list(s) == [k for k in s if k in w] and set(s) == set(w)
        assert all(isinstance(v, str) or v.dtype == torch.int64 for v in s.values())
        assert _plain(s) == w, i


def test_sequence_datasets_match_the_reference_exactly():
    from rec_pangu_amd.dataset import SequenceDataset, SequenceDatasetV2
    fx = load_json("sequence_dataset.json")
    first = SequenceDatasetV2(dict(fx["config"]), _frame(fx), phase="train")
    assert first.enc_dict == fx["enc_dict"]
    for phase in ("train", "valid", "test"):
        ds = SequenceDatasetV2(dict(fx["config"]), _frame(fx), enc_dict=fx["enc_dict"], phase=phase)
        _check_samples(ds, fx[f"v2_{phase}"])
        if phase != "train":
            assert ds.get_test_gd() == fx[f"v2_{phase}_gd"]
    ds = SequenceDataset(dict(fx["config"]), _frame(fx), enc_dict=fx["enc_dict"], phase="test")
    _check_samples(ds, fx["v1_test"])
    assert ds.get_test_gd() == fx["v1_test_gd"]
    ds = SequenceDataset(dict(fx["config"]), _frame(fx), enc_dict=fx["enc_dict"], phase="train")
    random.seed(0)
    _check_samples(ds, fx["v1_train_seed0"])


def test_sequence_dataset_shapes_and_collate():
    from rec_pangu_amd.dataset import SequenceDatasetV2, seq_collate
    fx = load_json("sequence_dataset.json")
    ds = SequenceDatasetV2(dict(fx["config"]), _frame(fx), phase="train")
    s = ds[0]
    assert s["hist_item_list"].shape == (10,) and s["target_item"].shape == (1,) and "next_item_list" not in s
    a, b, items = seq_collate([(ds[i]["hist_item_list"], ds[i]["hist_mask_list"], int(ds[i]["target_item"])) for i in range(3)])
    assert a.dtype == b.dtype == torch.int64 and a.shape == b.shape == (3, 10) and len(items) == 3
    assert torch.equal(a[1], ds[1]["hist_item_list"]) and torch.equal(b[2], ds[2]["hist_mask_list"])


# ---- evaluation -----------------------------------------------------------------------------------------------------------
def test_evaluate_recall_matches_the_reference_exactly():
    from rec_pangu_amd.utils.evaluate import evaluate_recall
    fx = load_json("evaluate_recall.json")
    assert "u4" not in fx["preds"] and "u4" in fx["test_gd"]  # a user without a prediction
    assert not set(fx["preds"]["u2"]) & set(fx["test_gd"]["u2"])  # a user without a hit
    for case in fx["cases"]:
        assert evaluate_recall(fx["preds"], fx["test_gd"], case["topN"]) == case["want"], case["topN"]
    # numpy rows (what a search returns) are accepted like lists
    as_np = {k: np.asarray(v) for k, v in fx["preds"].items()}
    assert evaluate_recall(as_np, fx["test_gd"], 5) == fx["cases"][2]["want"]


class StubRecallModel(torch.nn.Module):
    """user_emb = rows of a fixed table picked by data['row']: [B, D], or [B, interests, D]"""

    def __init__(self, items, users):
        super().__init__()
        self.items = torch.nn.Parameter(items)
        self.users = torch.nn.Parameter(users)

    def output_items(self):
        return self.items

    def forward(self, data, is_training=True):
        return {"user_emb": self.users[data["row"]]}


def gapped_recall_data(n_users, n_items, dim, topN, interests=0, seed=0, min_gap=1e-5):
    """float32 items / users whose float64 normalised scores have consecutive gaps above min_gap among each (user, interest)
    row's topN + 1 largest — ASSERTED here — so the order of the first topN is defined at fp32 precision.  Rows that miss the
    gap are redrawn; item 0 exists and is a zero row (stays zero under the normalisation)."""
    gen = torch.Generator().manual_seed(seed)
    items = torch.randn(n_items, dim, generator=gen)
    items[0] = 0
    rows = n_users * max(interests, 1)
    users = torch.randn(rows, dim, generator=gen)

    def scores64(u):
        i64, u64 = items.double(), u.double()
        i64 = i64 / torch.where(i64.norm(dim=1) == 0, torch.ones(()).double(), i64.norm(dim=1))[:, None]
        u64 = u64 / u64.norm(dim=1)[:, None]
        return u64 @ i64.t()

    def gaps(s):
        top = torch.sort(s, dim=1, descending=True).values[:, :topN + 1]
        return (top[:, :-1] - top[:, 1:]).min(dim=1).values

    for _ in range(200):
        bad = gaps(scores64(users)) <= min_gap
        if not bool(bad.any()):
            break
        users[bad] = torch.randn(int(bad.sum()), dim, generator=gen)
    s = scores64(users)
    assert float(gaps(s).min()) > min_gap
    if interests:
        users = users.reshape(n_users, interests, dim)
    return items, users, s


def expected_preds(s, n_users, topN, interests=0):
    """from the float64 scores: argsort per row; multi-interest: the reference's merge (all interests' topN by score, item 0
    and repeats dropped, the first topN kept)"""
    order = torch.argsort(s, dim=1, descending=True)[:, :topN]
    want = {}
    for u in range(n_users):
        if not interests:
            want[str(u)] = order[u].tolist()
            continue
        cand = []
        for r in range(u * interests, (u + 1) * interests):
            cand += [(int(i), float(s[r, i])) for i in order[r]]
        cand.sort(key=lambda x: x[1], reverse=True)
        chosen = []
        for item, _ in cand:
            if item not in chosen and item != 0:
                chosen.append(item)
            if len(chosen) >= topN:
                break
        want[str(u)] = chosen
    return want


def recall_loader(n_users, batch):
    out = []
    for lo in range(0, n_users, batch):
        rows = list(range(lo, min(lo + batch, n_users)))
        out.append({"user": [str(r) for r in rows], "row": torch.tensor(rows)})
    return out


@pytest.mark.parametrize("interests", [0, 3])
def test_get_recall_predict_on_cpu_against_float64_argsort(interests):
    from rec_pangu_amd.utils.evaluate import get_recall_predict
    n_users, n_items, dim, topN = 23, 301, 8, 20
    items, users, s = gapped_recall_data(n_users, n_items, dim, topN, interests)
    model = StubRecallModel(items, users)
    preds = get_recall_predict(model, recall_loader(n_users, 7), torch.device("cpu"), topN=topN)
    want = expected_preds(s, n_users, topN, interests)
    assert set(preds) == set(want) and len(preds) == n_users  # no user left out
    for u in want:
        assert list(preds[u]) == want[u], u
        assert all(isinstance(i, int) for i in preds[u])


def test_get_recall_predict_pads_a_small_vocabulary():
    from rec_pangu_amd.utils.evaluate import get_recall_predict
    items, users, s = gapped_recall_data(4, 6, 4, 5)
    preds = get_recall_predict(StubRecallModel(items, users), recall_loader(4, 4), torch.device("cpu"), topN=9)
    for u, row in preds.items():
        assert row[:6] == torch.argsort(s[int(u)], descending=True).tolist() and row[6:] == [-1, -1, -1]


# ---- trainer --------------------------------------------------------------------------------------------------------------
def _tiny_loaders(batch_size=4):
    import torch.utils.data as D_
    from rec_pangu_amd.dataset import SequenceDatasetV2
    fx = load_json("sequence_dataset.json")
    cfg = dict(fx["config"], cate_cols=[])
    train = SequenceDatasetV2(dict(cfg), _frame(fx), phase="train")
    valid = SequenceDatasetV2(dict(cfg), _frame(fx), enc_dict=train.enc_dict, phase="valid")
    test = SequenceDatasetV2(dict(cfg), _frame(fx), enc_dict=train.enc_dict, phase="test")
    mk = lambda ds, sh: D_.DataLoader(ds, batch_size=batch_size, shuffle=sh, num_workers=0)  # noqa: E731
    model_cfg = {"embedding_dim": 8, "max_length": cfg["max_length"], "device": "cpu", "item_col": "item_id", "cate_cols": []}
    return train.enc_dict, model_cfg, mk(train, True), mk(valid, False), mk(test, False)


def test_sequence_trainer_fit_writes_checkpoints_and_log(tmp_path):
    import inspect
    import pandas as pd
    from rec_pangu_amd.models.sequence import YotubeDNN
    from rec_pangu_amd.trainer import SequenceTrainer
    sig = inspect.signature(SequenceTrainer.fit).parameters
    assert list(sig) == ["self", "model", "train_loader", "valid_loader", "epoch", "lr", "device", "topk_list", "use_earlystoping",
                         "max_patience", "monitor_metric", "log_rounds", "lr_scheduler_type", "scheduler_params"]
    assert sig["epoch"].default == 50 and sig["max_patience"].default == 999 and sig["log_rounds"].default == 100
    assert list(inspect.signature(SequenceTrainer.__init__).parameters) == ["self", "wandb_config", "model_ckpt_dir"]
    enc, cfg, train, valid, test = _tiny_loaders()
    torch.manual_seed(0)
    model = YotubeDNN(enc, cfg)
    before = model.item_emb.weight.detach().clone()
    ckpt = str(tmp_path / "ckpt")
    trainer = SequenceTrainer(model_ckpt_dir=ckpt)
    trainer.fit(model, train, valid, epoch=2, lr=1e-2, device=torch.device("cpu"), topk_list=[5, 10],
                use_earlystoping=True, max_patience=5, monitor_metric="recall@10", log_rounds=1)
    assert not torch.equal(before, model.item_emb.weight.detach())
    for name in ("model_e_1.pth", "model_e_2.pth", "model_best.pth", "log.csv"):
        assert os.path.exists(os.path.join(ckpt, name)), name
    sd = torch.load(os.path.join(ckpt, "model_e_2.pth"))
    assert list(sd) == ["model"] and list(sd["model"]) == ["item_emb.weight"]
    log = pd.read_csv(os.path.join(ckpt, "log.csv"))
    assert len(log) == 2 and list(log["phase"]) == ["valid", "valid"]
    assert set(log.columns) == {"recall@5", "ndcg@5", "hitrate@5", "recall@10", "ndcg@10", "hitrate@10", "phase"}
    metric = trainer.evaluate_model(model, test, torch.device("cpu"), topk_list=[5])
    assert set(metric) == {"recall@5", "ndcg@5", "hitrate@5", "phase"} and metric["phase"] == "test"
    assert all(0.0 <= metric[k] <= 1.0 for k in metric if k != "phase")
    assert len(pd.read_csv(os.path.join(ckpt, "log.csv"))) == 3
    trainer.save_all(model, enc, ckpt)
    assert set(torch.load(os.path.join(ckpt, "model.pth"))) == {"model", "enc_dict"}


def test_sequence_trainer_stops_early_on_the_monitored_metric(tmp_path):
    from rec_pangu_amd.models.sequence import YotubeDNN
    from rec_pangu_amd.trainer import SequenceTrainer
    enc, cfg, train, valid, _ = _tiny_loaders()
    torch.manual_seed(0)
    trainer = SequenceTrainer(model_ckpt_dir=str(tmp_path))
    # lr = 0: the metric cannot improve after the first epoch -> patience 1 stops at epoch 2 of 5
    trainer.fit(YotubeDNN(enc, cfg), train, valid, epoch=5, lr=0.0, topk_list=[10], use_earlystoping=True, max_patience=1,
                monitor_metric="hitrate@10")
    assert len(trainer.log_df) == 2 and not os.path.exists(os.path.join(str(tmp_path), "model_e_3.pth"))
    with pytest.raises(AssertionError):
        trainer.fit(YotubeDNN(enc, cfg), train, valid, epoch=1, topk_list=[10], use_earlystoping=True, monitor_metric="auc")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ["rp_softmax_ce_geometry", "rp_softmax_ce_splits", "rp_softmax_ce_workspace_bytes", "rp_softmax_ce_fwd",
               "rp_softmax_ce_bwd", "rp_hist_mean_fwd", "rp_hist_mean_bwd"]


def test_new_symbols_are_declared_bound_and_exported():
    from rec_pangu_amd import hip
    assert hip.ABI_VERSION == 108
    header = open(os.path.join(ROOT, "include", "rec_pangu_hip.h")).read()
    lib = hip.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, f"{name} is not declared in the header"
        assert name in hip.EXPORTED_SYMBOLS and len(hip._SIGNATURES[name][1]) == m.group(1).count(",") + 1, name
        getattr(lib, name)
    assert lib.rp_version() == 108


def test_softmax_ce_geometry_and_split_rule():
    from rec_pangu_amd import hip
    g = hip.softmax_ce_geometry()
    assert g["TB"] >= 1 and g["TV"] >= 1 and g["slices"] >= 1 and g["max_d"] >= 64
    assert hip.softmax_ce_fits(1) and hip.softmax_ce_fits(g["max_d"]) and not hip.softmax_ce_fits(g["max_d"] + 1)
    for B, Vv in [(1, 2), (33, 70000), (4096, 2 ** 20), (65536, 2 ** 17)]:
        n, per = hip.softmax_ce_splits(B, Vv)
        tiles = -(-Vv // g["TV"])
        assert n >= 1 and (n - 1) * per < tiles <= n * per, (B, Vv, n, per)  # every split holds a tile, together all of them
    assert hip.softmax_ce_splits(1, g["TV"])[0] == 1


def test_score_tile_split_plan_and_workspaces_keep_their_values():
    """the host side of the two score-tile losses (split plan and workspace layouts), which no device listing covers: the
    values of the build before the plan moved into csrc/score_tile.h.  (1, 32) and (5, 129) sit on the MIN_TILES floor,
    (33, 70000) under the MAX_SPLITS cap, (4096, 131072) at the FILL target, (65536, 131072) needs no split."""
    from rec_pangu_amd import hip
    # (rows, cols): (splits, tiles per split), {D: (softmax-CE workspace bytes, contrastive workspace bytes)}
    pinned = {
        (1, 32): ((1, 4), {12: (72, 128), 128: (536, 1056)}),
        (5, 129): ((2, 4), {12: (576, 896), 128: (5216, 7856)}),
        (33, 70000): ((63, 35), {12: (116440, 134656), 128: (1081096, 1114624)}),
        (4096, 131072): ((8, 512), {12: (1835264, 2293824), 128: (17039616, 19398720)}),
        (65536, 131072): ((1, 4096), {12: (3674112, 7341056), 128: (34082816, 68158464)}),
    }
    for (rows, cols), (splits, ws) in pinned.items():
        assert tuple(hip.softmax_ce_splits(rows, cols)) == splits, (rows, cols)
        for Dd, (sce, ctr) in ws.items():
            assert hip.softmax_ce_workspace_bytes(rows, cols, Dd) == sce, (rows, cols, Dd)
            assert hip.contrast_workspace_bytes(rows, cols, Dd) == ctr, (rows, cols, Dd)
    assert hip.softmax_ce_geometry() == {"TB": 32, "TV": 32, "max_d": 128, "slices": 4}
    assert hip.contrast_geometry() == {"TA": 32, "TB": 32, "max_d": 128, "max_splits": 64}


def test_softmax_ce_workspace_does_not_hold_the_logits():
    """a condition on the design: at B = 4096, V = 2^20, D = 64 the workspace is below 1/16 of the 16 GiB logits, and what
    grows with B alone is linear in B"""
    from rec_pangu_amd import hip
    B, Vv, Dd = 4096, 2 ** 20, 64
    ws = hip.softmax_ce_workspace_bytes(B, Vv, Dd)
    assert 0 < ws < (4 * B * Vv) // 16
    assert hip.softmax_ce_workspace_bytes(B, 2 * Vv, Dd) <= 2 * ws  # (more tiles per split, not more splits per row)
    assert hip.softmax_ce_workspace_bytes(65536, 2 ** 17, Dd) < (4 * 65536 * 2 ** 17) // 16


def test_softmax_ce_entry_points_reject_bad_arguments():
    from rec_pangu_amd import hip
    lib = hip.lib()
    n = ctypes.c_size_t(0)
    assert lib.rp_softmax_ce_workspace_bytes(0, 5, 4, ctypes.byref(n)) == -1
    assert lib.rp_softmax_ce_workspace_bytes(4, 5, 4, None) == -1
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    big_d = hip.softmax_ce_geometry()["max_d"] + 1
    # D above the budget and ldu < D are refused before anything is launched (host pointers are never dereferenced)
    assert lib.rp_softmax_ce_fwd(p, big_d, p, p, 1, 2, big_d, p, p, p, p, 1 << 20, None) == -1
    assert b"register budget" in lib.rp_last_error()
    assert lib.rp_softmax_ce_fwd(p, 2, p, p, 1, 2, 4, p, p, p, p, 1 << 20, None) == -1
    assert lib.rp_softmax_ce_bwd(p, 4, p, p, p, p, 1, 2, 4, None, 0, None, p, 1 << 20, None) == -1  # neither gradient
    assert lib.rp_hist_mean_fwd(p, 3, 4, p, p, 2, 0, p, 4, p, None) == -1
    assert lib.rp_hist_mean_bwd(p, p, 4, 2, 4, 3, p, p, 2, p, None) == -1
