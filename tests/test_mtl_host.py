"""ESSM / AITM on the CPU (plumbing, no GPU): state_dict contract, init RNG stream and forward / backward / Adam numerics against
the golden vectors produced by running the reference (tests/golden/make_golden_mtl.py), the constructor and loss signatures,
the trainer registry, prediction shapes, RankTrainer / BenchmarkTrainer with num_task = 2, and the argument validation of the
pair-loss and wide-attention entry points."""
import ctypes
import inspect
import os

import pandas as pd
import pytest
import torch

from conftest import GOLDEN, load_golden, small_enc_dict

torch.set_num_threads(1)

# the first model seed from 1234 upward at which every ReLU pre-activation and AITM's p2 - p1 clear 1e-5 at the three recorded
# states of all four cases, each side of the constraint holding at least 3 rows: as tests/golden/make_golden_mtl.py printed it
SEED = 3120
CASES = {  # fixture -> (class name, constructor arguments, train mode)
    "essm_eval": ("ESSM", dict(embedding_dim=8, hidden_dim=[8, 4], dropouts=[0.2, 0.2]), False),
    "essm_train": ("ESSM", dict(embedding_dim=8, hidden_dim=[8, 4], dropouts=[0.0, 0.0]), True),
    "aitm_eval": ("AITM", dict(embedding_dim=8, tower_dims=[16, 8, 12], drop_prob=[0.1, 0.1, 0.1]), False),
    "aitm_train": ("AITM", dict(embedding_dim=8, tower_dims=[16, 8, 12], drop_prob=[0.0, 0.0, 0.0]), True),
}
MTL_NAMES = ["MMOE", "OMOE", "MLMMOE", "ShareBottom", "ESSM", "AITM"]  # the reference's multi-task model list


def build(case):
    from rec_pangu_amd.models import multi_task
    name, kw, train_mode = CASES[case]
    torch.manual_seed(SEED)
    model = getattr(multi_task, name)(enc_dict=small_enc_dict(), **kw)
    model.train(train_mode)
    return model


@pytest.mark.parametrize("case", list(CASES))
def test_init_stream_and_state_dict_contract(case):
    g = load_golden(f"model_{case}.npz")
    sd = build(case).state_dict()
    assert list(sd.keys()) == list(g["init"].keys())
    for k, v in g["init"].items():
        assert sd[k].shape == v.shape, k
        assert torch.equal(sd[k], v), f"{case}: init of {k} differs from the reference's"
    tops = list(dict.fromkeys(k.split(".")[0] for k in sd if not k.startswith("embedding_layer.")))
    if case.startswith("essm"):
        assert tops == ["ctr_layer", "cvr_layer"]
    else:
        assert tops == ["click_tower", "conversion_tower", "attention_layer", "info_layer", "click_layer", "conversion_layer"]
        assert [k for k in sd if k.startswith("attention_layer.")] == [f"attention_layer.W_{p}.weight" for p in "qkv"]
    assert "after1" not in g, "no BatchNorm in these models: no running statistics to pin"


@pytest.mark.parametrize("case", list(CASES))
def test_forward_backward_adam_vs_reference(case):
    g = load_golden(f"model_{case}.npz")
    model = build(case)
    out = model({k: v.clone() for k, v in g["batch"].items()})
    assert set(out) == set(g["out"])
    for k, v in g["out"].items():
        assert out[k].shape == v.shape, k
        torch.testing.assert_close(out[k].detach(), v, rtol=1e-5, atol=1e-6, msg=lambda m: f"{case}:{k}: {m}")
    model.zero_grad()
    out["loss"].backward()
    params = dict(model.named_parameters())
    assert set(g["grad"]) == set(params), "every parameter receives a gradient"
    for k, v in g["grad"].items():
        torch.testing.assert_close(params[k].grad, v, rtol=1e-4, atol=1e-6, msg=lambda m: f"{case}:grad {k}: {m}")
    model = build(case)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, betas=(0.9, 0.999), eps=1e-08, weight_decay=0)
    for _ in range(2):
        r = model({k: v.clone() for k, v in g["batch"].items()})
        r["loss"].backward()
        opt.step()
        model.zero_grad()
    sd = model.state_dict()
    for k, v in g["adam2"].items():
        torch.testing.assert_close(sd[k], v, rtol=1e-4, atol=1e-6, msg=lambda m: f"{case}:adam2 {k}: {m}")
    model.eval()
    with torch.no_grad():
        r = model({k: v.clone() for k, v in g["batch"].items()}, is_training=False)
    assert "loss" not in r
    for k, v in g["adam2_out"].items():
        torch.testing.assert_close(r[k], v, rtol=1e-5, atol=1e-6)


def test_prediction_shapes():
    batch = load_golden("model_essm_eval.npz")["batch"]
    B = batch["task1_label"].shape[0]
    for case in CASES:
        out = build(case)(dict(batch))
        want = (B, 1) if case.startswith("essm") else (B,)
        assert out["task1_pred"].shape == want and out["task2_pred"].shape == want and out["loss"].shape == ()


def test_signatures_and_registry():
    """the signatures as inspect.signature gives them for the reference's classes (essm.py:13-18,69; aitm.py:15-19,84-89)"""
    from rec_pangu_amd.benchmark_trainer import MODEL_REGISTRY
    from rec_pangu_amd.models import multi_task
    from rec_pangu_amd.models.multi_task import AITM, ESSM

    def sig(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if k != "self"}

    E = inspect.Parameter.empty
    assert sig(ESSM.__init__) == dict(embedding_dim=40, hidden_dim=[128, 64], dropouts=[0.2, 0.2], enc_dict=None, device=None)
    assert list(sig(ESSM.__init__)) == ["embedding_dim", "hidden_dim", "dropouts", "enc_dict", "device"]
    assert sig(AITM.__init__) == dict(embedding_dim=32, tower_dims=[400, 400, 400], drop_prob=[0.1, 0.1, 0.1], enc_dict=None)
    assert list(sig(AITM.__init__)) == ["embedding_dim", "tower_dims", "drop_prob", "enc_dict"]
    assert sig(ESSM.loss) == dict(click=E, conversion=E, data=E, weight=0.5)
    assert list(sig(ESSM.loss)) == ["click", "conversion", "data", "weight"]
    assert sig(AITM.loss) == dict(click_label=E, click_pred=E, conversion_label=E, conversion_pred=E, constraint_weight=0.6)
    assert list(sig(AITM.loss)) == ["click_label", "click_pred", "conversion_label", "conversion_pred", "constraint_weight"]
    assert sig(ESSM.forward) == sig(AITM.forward) == dict(data=E, is_training=True)
    assert multi_task.__all__ == MTL_NAMES
    assert MODEL_REGISTRY["ESSM"] is ESSM and MODEL_REGISTRY["AITM"] is AITM
    model = AITM(enc_dict=small_enc_dict())
    att = model.attention_layer
    assert (att.num_heads, att.attention_dim, att.W_res, att.scale) == (1, 400, None, None)
    assert [type(m).__name__ for m in model.info_layer] == ["Linear", "ReLU", "Dropout"] and model.info_layer[2].p == 0.1
    assert [type(m).__name__ for m in model.click_layer] == ["Linear", "Sigmoid"]
    assert [type(m).__name__ for m in ESSM(enc_dict=small_enc_dict()).ctr_layer.net] == \
        ["Linear", "ReLU", "Dropout", "Linear", "ReLU", "Dropout", "Linear"]


def test_the_losses_on_cpu_tensors_are_the_reference_formulas():
    from rec_pangu_amd.models.multi_task import AITM, ESSM
    g = torch.Generator().manual_seed(0)
    p1, p2 = torch.rand(40, generator=g), torch.rand(40, generator=g)
    y1, y2 = (torch.rand(40, generator=g) < 0.4).float(), (torch.rand(40, generator=g) < 0.2).float()
    bce = torch.nn.functional.binary_cross_entropy
    essm, aitm = ESSM(enc_dict=small_enc_dict()), AITM(enc_dict=small_enc_dict(), tower_dims=[8, 8], drop_prob=[0.1, 0.1])
    data = {"task1_label": y1, "task2_label": y2}
    assert torch.equal(essm.loss(p1[:, None], (p1 * p2)[:, None], data), bce(p1 * p2, y2) + 0.5 * bce(p1, y1))
    assert torch.equal(essm.loss(p1[:, None], p2[:, None], data, weight=0.25), bce(p2, y2) + 0.25 * bce(p1, y1))
    assert torch.equal(aitm.loss(y1, p1, y2, p2), bce(p1, y1) + bce(p2, y2) + 0.6 * (p2 - p1).clamp(min=0).sum())
    assert torch.equal(aitm.loss(y1, p1, y2, p2, constraint_weight=2.0),
                       bce(p1, y1) + bce(p2, y2) + 2.0 * (p2 - p1).clamp(min=0).sum())


def _multitask_loaders():
    from rec_pangu_amd.dataset import get_dataloader
    import json
    meta = json.load(open(os.path.join(GOLDEN, "dataset.json")))
    df = pd.read_json(os.path.join(GOLDEN, "dataset_frame.json"), orient="split")
    schema = dict(meta["schema"], label_col=["click", "scroll"], task_type="multitask")
    return get_dataloader(df[:100].copy(), df[100:130].copy(), df[130:].copy(), schema, batch_size=50)


@pytest.mark.parametrize("name", ["ESSM", "AITM"])
def test_rank_trainer_fit_and_evaluate(name, tmp_path):
    from rec_pangu_amd.benchmark_trainer import MODEL_REGISTRY
    from rec_pangu_amd.trainer import RankTrainer
    train_loader, valid_loader, test_loader, enc = _multitask_loaders()
    torch.manual_seed(0)
    kw = dict(hidden_dim=[8, 4]) if name == "ESSM" else dict(tower_dims=[8, 8], drop_prob=[0.1, 0.1])
    model = MODEL_REGISTRY[name](embedding_dim=4, enc_dict=enc, **kw)
    trainer = RankTrainer(num_task=2, model_ckpt_dir=str(tmp_path))
    keys = {f"task{i}_{m}" for i in (1, 2) for m in ("roc_auc_score", "log_loss")}
    assert set(trainer.fit(model, train_loader, valid_loader, epoch=1, lr=1e-3)) == {f"test_{k}" for k in keys}
    assert set(trainer.evaluate_model(model, test_loader)) == {f"test_{k}" for k in keys}
    from rec_pangu_amd.model_pipeline import train_model
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    assert set(train_model(model, train_loader, opt, torch.device("cpu"), num_task=2)) == {f"train_{k}" for k in keys}


def test_benchmark_trainer_runs_the_reference_multitask_list(tmp_path):
    from rec_pangu_amd.benchmark_trainer import BenchmarkTrainer
    train_loader, valid_loader, test_loader, enc = _multitask_loaders()
    csv = os.path.join(tmp_path, "mt.csv")
    bt = BenchmarkTrainer(num_task=2, model_list=MTL_NAMES, benchmark_res_path=csv, ckpt_root=os.path.join(tmp_path, "ck"))
    bt.run(train_loader, enc, valid_loader, test_loader, epoch=1, lr=1e-3, device=torch.device("cpu"))
    res = pd.read_csv(csv)
    assert list(res["model_name"]) == MTL_NAMES
    assert {"test_task1_roc_auc_score", "test_task2_log_loss", "train_model_time"} <= set(res.columns)
    assert res.notna().all().all()


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    from rec_pangu_amd import hip
    lib = hip.lib()
    assert lib.rp_version() == hip.ABI_VERSION == 108  # (no existing prototype changed)
    new = ("rp_pair_loss_fwd", "rp_pair_loss_bwd", "rp_attention_wide_fits", "rp_attention_wide_fwd", "rp_attention_wide_bwd")
    assert all(name in hip.EXPORTED_SYMBOLS for name in new)
    assert lib.rp_attention_wide_fits(2, 1, 400) == 1 and lib.rp_attention_wide_fits(2, 2, 200) == 0
    assert all(hip.attention_wide_fits(T, 1, a) for T in (2, 3, 4) for a in (1, 20, 64, 68, 400, 1024, 65536))
    assert not any(hip.attention_wide_fits(*c) for c in ((1, 1, 400), (5, 1, 400), (2, 1, 0), (2, 1, 65537), (2, 0, 8)))
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # null pointers and an empty batch are refused with an error code and a message, never a crash
    assert lib.rp_pair_loss_fwd(None, None, None, None, 4, 0, 0.5, 1, None, None, None, None, None) == -1
    assert b"null" in lib.rp_last_error()
    assert lib.rp_pair_loss_fwd(p, p, p, p, 0, 0, 0.5, 1, p, p, p, p, None) == -1 and b"empty" in lib.rp_last_error()
    assert lib.rp_pair_loss_fwd(p, p, p, p, 4, 2, 0.5, 1, p, p, p, p, None) == -1 and b"mode" in lib.rp_last_error()
    assert lib.rp_pair_loss_bwd(None, None, None, None, None, 4, 1, 0.6, 1, None, None, None) == -1
    assert b"null" in lib.rp_last_error()
    assert lib.rp_pair_loss_bwd(p, p, p, p, p, 0, 1, 0.6, 1, p, p, None) == -1 and b"empty" in lib.rp_last_error()
    assert lib.rp_pair_loss_bwd(p, p, p, p, p, 4, -1, 0.6, 1, p, p, None) == -1 and b"mode" in lib.rp_last_error()
    assert lib.rp_attention_wide_fwd(None, 0, None, 0, 2, 1, 8, 0.0, 1, None, 4, None) == -1 and b"null" in lib.rp_last_error()
    assert lib.rp_attention_wide_fwd(p, 24, p, 8, 2, 1, 8, 0.0, 1, p, 0, None) == -1 and b"empty" in lib.rp_last_error()
    assert lib.rp_attention_wide_fwd(p, 23, p, 8, 2, 1, 8, 0.0, 1, p, 4, None) == -1 and b"leading" in lib.rp_last_error()
    assert lib.rp_attention_wide_fwd(p, 24, p, 7, 2, 1, 8, 0.0, 1, p, 4, None) == -1 and b"leading" in lib.rp_last_error()
    assert lib.rp_attention_wide_fwd(p, 24, p, 8, 2, 2, 4, 0.0, 1, p, 4, None) == -3  # H != 1
    assert lib.rp_attention_wide_fwd(p, 24, p, 8, 5, 1, 8, 0.0, 1, p, 4, None) == -3  # T > 4
    assert lib.rp_attention_wide_bwd(None, 0, None, 0, None, 2, 1, 8, 0.0, 1, None, 0, None, 0, 4, None) == -1
    assert b"null" in lib.rp_last_error()
    assert lib.rp_attention_wide_bwd(p, 24, p, 8, p, 2, 1, 8, 0.0, 1, p, 24, p, 8, 0, None) == -1
    assert b"empty" in lib.rp_last_error()
    assert lib.rp_attention_wide_bwd(p, 24, p, 8, p, 2, 1, 8, 0.0, 1, p, 23, p, 8, 4, None) == -1
    assert b"leading" in lib.rp_last_error()
    assert lib.rp_attention_wide_bwd(p, 24, p, 8, p, 2, 3, 8, 0.0, 1, p, 24, p, 8, 4, None) == -3
    # the wrappers' checks come before anything touches a device
    z = torch.zeros(8)
    with pytest.raises(RuntimeError, match="HIP-device"):
        hip.pair_loss_fwd(z, z, z, z, hip.PAIR_ESSM, 0.5)
    with pytest.raises(RuntimeError, match="HIP-device"):
        hip.attention_wide_fwd(torch.zeros(4, 24), torch.zeros(4, 8), 2, 8, 0.0, True)
