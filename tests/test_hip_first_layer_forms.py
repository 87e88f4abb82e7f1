"""Every form of embed_gather_linear_kernel (csrc/embed.hip) run alone on the device against first_layer_f64, the float64
statement of tests/test_first_layer_host.py, over that file's cases.  embed_gather_linear_launch issues six instantiations
<FULL, STORE_X, BF16_ROWS>; a test id names the ones its case reaches:

    full_x    <true, true>    B >= 128 and x (fp32 rows) / x_bf16 (bf16 rows) given
    full_nox  <true, false>   B >= 128, x not stored: only xd (training, "dense") or nothing (inference, "none" / "infer")
    tail_x    <false, true>   B % 128 != 0, the masked last workgroup, x given
    tail_nox  <false, true>   the same instantiation with x = NULL
  each over an fp32 arena (f32) or a bf16 arena (bf16).

Asserted per case and form: keys, x / x_bf16 / xd bit-exact (the dense columns of x_bf16 = dense.to(bfloat16), exact zeros in
every padding column); h1, ssum, fm inside the host file's bars, the bf16 forms against the reference built from the
bf16-rounded table (the kernel adds no bf16 rounding of its own); two launches bit-identical; h1 / fm / ssum / keys
bit-identical whether or not sum_out / keys_out were requested, between x_mode full / dense / none and between the three
bf16 forms; the fp32 form over arena16.float() within twice the h1 bar of the bf16 form; a sample's results bit-identical
wherever it sits in the batch; NaN in every arena row nobody looks up, behind column K of W and behind W's last row changes
nothing; no row >= B of any output is written and every live element is; an id outside its table raises the flag in every
form and reads as row 0; what the launch refuses it refuses without a launch.

Worst error as a share of its bar, per form (printed by every test, and per form at the end of the module: run with -s),
as observed on the MI355X; h1 = where |pre| is clear of zero (bar 2e-5 max|pre|), h1-all = everywhere (4e-5 max|pre|):
  fp32 rows   full / dense / none   h1 0.087  h1-all 0.043  ssum 0.065  fm 0.001   (the three forms gave the same bits)
  bf16 rows   x16 / xd / infer      h1 0.061  h1-all 0.030  ssum 0.008  fm 0.000
  the fp32 form over arena16.float() against the bf16 form: h1 bit-identical in all 31 cases
  the dense k-step on one-hot dense columns: h1 = relu(w) bit for bit in the four forms that run it
No form lands above a tenth of a bar, and no assertion found the kernel wrong.
"""
import functools
import itertools

import pytest
import torch

from conftest import require_gpu
from test_first_layer_host import (BAD_CASE, BAD_IDS, CASES, D, bad_ids, case_inputs, case_reference, fm_share, h1_shares,
                                   first_layer_f64, first_layer_inputs, ssum_share)

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
F32_FORMS, BF16_FORMS = ("full", "dense", "none"), ("x16", "xd", "infer")
LDX4_CASES = {(129, 5, 13), (37, 2, 0)}  # also run with ldx = K rounded up to 4: padding of 3 and of 0 columns
CANARY_F32, CANARY_I32, CANARY_I16 = -12345.6789, 0x5A5A5A5A, 0x5A5A
GUARD_ROWS = 128
WORST = {}  # form -> tensor -> worst share of its bar


@pytest.fixture(scope="module")
def hip():
    require_gpu()
    from rec_pangu_amd import hip as h
    h.lib()
    h.set_matmul_precision("bf16x6")
    try:
        yield h
    finally:
        h.set_matmul_precision("auto")
        for form in sorted(WORST):
            print(f"\nworst share of bar, {form}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(WORST[form].items())), end="")
        print()


def reached(B, stores_x, bf16_rows):
    """the instantiations a batch of B reaches, as the test id spells them"""
    tag = "x" if stores_x else "nox"
    parts = (["full_" + tag] if B >= 128 else []) + (["tail_" + tag] if B % 128 else [])
    return ("bf16-" if bf16_rows else "f32-") + "+".join(parts)


def form_id(case, form):
    return "B%d-F%d-ND%d-" % case + form + "-" + reached(case[0], form in ("full", "x16"), form in BF16_FORMS)


def bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def round_up(n, m):
    return (n + m - 1) // m * m


@functools.lru_cache(maxsize=None)
def dev_case(case):
    """the case's inputs on the device: uploaded once, shared, left unchanged.  W is a [64, K] view with ldw = K rounded up
    to 4 floats per row (exactly K where K % 4 == 0), zeros behind column K"""
    B, F, ND = case
    inp = case_inputs(case)
    K = F * D + ND
    ldw = round_up(K, 4)
    wbuf = torch.zeros(64, ldw, device=DEV)
    wbuf[:, :K] = inp["W"].to(DEV)
    return {"arena": inp["arena"].to(DEV), "arena16": inp["arena"].to(torch.bfloat16).to(DEV),
            "rb": torch.tensor(inp["base"], dtype=torch.int64, device=DEV),
            "rc": torch.tensor(inp["rows"], dtype=torch.int64, device=DEV),
            "idx": [t.to(DEV) for t in inp["idx"]], "dense": [t.to(DEV) for t in inp["dense"]],
            "W": wbuf[:, :K], "ldw": ldw, "bias": inp["bias"].to(DEV), "K": K}


def new_flag():
    return torch.zeros(2, dtype=torch.int32, device=DEV)


def run_wrapper(hip, d, form, ldx, want_sum=True, want_keys=True, biased=True, idx=None, dense=None, arena=None, err=None):
    """one launch through hip.py -> (x | x_bf16 | xd | None, h1, fm [B], ssum, keys, err_flag); exactly one launch is counted"""
    idx, dense = idx or d["idx"], d["dense"] if dense is None else dense
    bias = d["bias"] if biased else None
    err = new_flag() if err is None else err
    n0 = hip.launch_count()
    if form in F32_FORMS:
        x, h1, fm, ssum, keys = hip.embed_gather_linear_fwd(d["arena"] if arena is None else arena, d["rb"], d["rc"], idx, dense, ldx,
                                                            d["W"], bias, True, want_sum, want_keys, err, x_mode=form)
    elif form == "infer":
        h1, fm = hip.embed_gather_linear_fwd_bf16(d["arena16"] if arena is None else arena, d["rb"], d["rc"], idx, dense, d["W"],
                                                  bias, err)
        x = ssum = keys = None
    else:
        x, h1, fm, ssum, keys = hip.embed_gather_linear_fwd_bf16(d["arena16"] if arena is None else arena, d["rb"], d["rc"], idx,
                                                                 dense, d["W"], bias, err, train_ldx=ldx, want_keys=want_keys,
                                                                 dense_only=form == "xd")
    assert hip.launch_count() - n0 == 1
    return x, h1, fm.reshape(-1), ssum, keys, err


def note(form, worst, name, share):
    worst[name] = max(worst.get(name, 0.0), share)
    per_form = WORST.setdefault(form, {})
    per_form[name] = max(per_form.get(name, 0.0), share)


def check_results(form, ref, out, worst):
    """h1 / fm / ssum against their bars, keys exact; absent outputs are skipped"""
    _, h1, fm, ssum, keys, _ = out
    assert h1.shape == ref["pre"].shape and bool(torch.isfinite(h1).all()) and bool((h1 >= 0).all())
    clear, everywhere = h1_shares(h1, ref)
    note(form, worst, "h1", clear)
    note(form, worst, "h1-all", everywhere)
    if fm is not None:
        note(form, worst, "fm", fm_share(fm, ref))
    if ssum is not None:
        note(form, worst, "ssum", ssum_share(ssum, ref))
    if keys is not None:
        assert keys.dtype == torch.int32 and torch.equal(keys.cpu(), ref["keys"]), "keys"


def check_stored(case, d, form, ref, x, ldx):
    """what the form stores of the activation: bit-exact copies, exact zeros in the padding"""
    B, F, ND = case
    K = d["K"]
    dense = torch.stack(d["dense"], dim=1) if ND else torch.zeros(B, 0, device=DEV)
    if form in ("none", "infer"):
        assert x is None
    elif form in ("dense", "xd"):  # xd [B, 64]: the dense columns in fp32 (also over bf16 rows), zeros up to 64
        assert x.dtype == torch.float32 and x.shape == (B, 64)
        assert same_bits(x[:, :ND], dense), "xd: dense columns"
        assert not bool(bits(x[:, ND:]).any()), "xd: padding is not exact zeros"
    elif form == "full":
        assert x.dtype == torch.float32 and x.shape == (B, ldx)
        assert same_bits(x[:, :K], ref["x"].float().to(DEV)), "x: rows / dense columns"
        assert not bool(bits(x[:, K:]).any()), "x: padding is not exact zeros"
    else:
        assert x.dtype == torch.bfloat16 and x.shape == (B, ldx)
        rows = d["arena16"][ref["keys"].to(DEV).long().view(F, B).T].reshape(B, F * D)
        assert same_bits(x[:, :F * D], rows), "x_bf16: embedding columns"
        assert same_bits(x[:, F * D:K], dense.to(torch.bfloat16)), "x_bf16: dense columns are dense.to(bfloat16)"
        assert not bool(bits(x[:, K:]).any()), "x_bf16: padding is not exact zeros"


def agree(a, b, what):
    """h1 / fm / ssum / keys of two launches bit-identical, wherever both have them"""
    for name, u, v in zip(("x", "h1", "fm", "ssum", "keys"), a[:5], b[:5]):
        if name != "x" and u is not None and v is not None:
            assert same_bits(u, v), f"{name} differs between {what}"


FORM_CASES = [(c, f) for c in CASES for f in F32_FORMS + BF16_FORMS]


@pytest.mark.parametrize("case,form", FORM_CASES, ids=[form_id(c, f) for c, f in FORM_CASES])
def test_form_against_float64(hip, case, form):
    B, F, ND = case
    d = dev_case(case)
    K = d["K"]
    bf16_rows = form in BF16_FORMS
    ldxs = [round_up(K, 64)] + ([round_up(K, 4)] if case in LDX4_CASES and form in ("full", "x16") else [])
    sums = (True, False) if form in F32_FORMS else (True,)  # (the bf16 wrapper's training forms always take the field sums)
    keyss = (True, False) if form != "infer" else (False,)
    worst = {}
    for biased in (True, False):
        ref = case_reference(case, bf16_rows, biased)
        first = None
        for ldx, want_sum, want_keys in itertools.product(ldxs, sums, keyss):
            out = run_wrapper(hip, d, form, ldx, want_sum, want_keys, biased)
            again = run_wrapper(hip, d, form, ldx, want_sum, want_keys, biased)
            assert int(out[5][0]) == 0 and int(again[5][0]) == 0, "err_flag on a clean batch"
            if form == "infer":
                assert out[3] is None and out[4] is None
            else:
                assert (out[3] is not None) == want_sum and (out[4] is not None) == want_keys
            check_results(form, ref, out, worst)
            check_stored(case, d, form, ref, out[0], ldx)
            agree(out, again, "two launches")
            if out[0] is not None:
                assert same_bits(out[0], again[0]), "the stored activation differs between two launches"
            first = first or out
            agree(first, out, "launches with and without sum_out / keys_out (the templates differ only in their stores)")
    print(f"\n{form_id(case, form)}: share of bar " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()), end="")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("case", CASES, ids=["B%d-F%d-ND%d" % c for c in CASES])
def test_forms_agree_bit_for_bit(hip, case):
    """the six instantiations differ in their loads' width and in their stores, not in their arithmetic: h1, fm, ssum, keys
    are bit-identical between x_mode full / dense / none, and between the three bf16 forms.  The fp32 form over the widened
    bf16 table against the bf16 form: h1 within twice its bar (the FM sums are laid out over 16 against 8 lanes there: they
    are held to their float64 bars, by test_form_against_float64)."""
    d = dev_case(case)
    ldx = round_up(d["K"], 64)
    f32 = [run_wrapper(hip, d, form, ldx) for form in F32_FORMS]
    agree(f32[0], f32[1], "x_mode full and dense")
    agree(f32[0], f32[2], "x_mode full and none")
    b16 = [run_wrapper(hip, d, form, ldx) for form in BF16_FORMS]
    agree(b16[0], b16[1], "bf16 rows with x_bf16 and with xd")
    agree(b16[0], b16[2], "bf16 rows, training and inference")
    assert same_bits(b16[0][4], f32[0][4]), "keys differ between fp32 and bf16 rows"
    widened = run_wrapper(hip, d, "none", ldx, arena=d["arena16"].float())
    pre = case_reference(case, True, True)["pre"].to(DEV)
    scale = float(pre.abs().max())
    err = (widened[1].double() - b16[0][1].double()).abs()
    clear = pre.abs() > 1e-5 * scale
    share = max(float((err * clear).max()) / (2 * 2e-5 * scale), float(err.max()) / (2 * 4e-5 * scale))
    print(f"\nB{case[0]}-F{case[1]}-ND{case[2]}: fp32 form over the widened bf16 table vs bf16 form, h1 share of twice the bar "
          f"{share:.3f}" + (" (bit-identical)" if same_bits(widened[1], b16[0][1]) else ""), end="")
    assert share <= 1.0


@pytest.mark.parametrize("form", ["full", "dense", "x16", "xd"])
def test_a_sample_does_not_depend_on_its_position(hip, form):
    """B = 421, F = 5, ND = 13, then the same batch in reversed order: every sample changes workgroup, wave and lane, the 37
    tail samples of one run sit in full workgroups of the other.  Every product and sum of a sample is taken in the same
    order wherever it sits: bit-identical rows."""
    case = (421, 5, 13)
    B, F, ND = case
    d = dev_case(case)
    ldx = round_up(d["K"], 64)
    fwd = run_wrapper(hip, d, form, ldx)
    rev = run_wrapper(hip, d, form, ldx, idx=[t.flip(0).contiguous() for t in d["idx"]],
                      dense=[t.flip(0).contiguous() for t in d["dense"]])
    assert int(fwd[5][0]) == 0 and int(rev[5][0]) == 0
    for name, pos in (("h1", 1), ("fm", 2), ("ssum", 3)):
        assert same_bits(fwd[pos], rev[pos].flip(0)), f"{name} of a sample depends on its position in the batch"
    assert torch.equal(fwd[4].view(F, B), rev[4].view(F, B).flip(1)), "keys"
    assert same_bits(fwd[0], rev[0].flip(0)), "the stored activation"
    worst = {}
    check_results(form, case_reference(case, form in BF16_FORMS, True), fwd, worst)
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("form", ["dense", "none", "xd", "infer"])
def test_dense_k_step_keeps_every_bit_of_w(hip, form):
    """The float64 bars cannot see the LAST bf16 piece of W (2^-17 of |w| per term against 2e-5 max|pre|); this can.  All-zero
    tables, no bias, and sample b's dense columns one-hot at column b % 16: pre[b, n] = W[n, F 64 + b % 16], a single
    product 1 x w.  1 splits into the pieces (1, 0, 0), w into three pieces of 8 significant bits whose sum is w exactly, so
    the accumulator adds at most three non-zero terms, multiples of ulp(w) with partial sums no larger than |w| (1 + 2^-8):
    smallest first every partial sum is representable and h1 = relu(w) bit for bit; in any order at most one addition
    rounds, by one ulp of the next binade: |h1 - relu(w)| <= 2^-22 |w|.  A dropped third piece leaves up to 2^-16 |w|.
    B = 160: one full workgroup and a 32-sample tail; W and -W, so that the ReLU lets every entry through once."""
    B, F, ND = 160, 2, 16
    inp = first_layer_inputs((B, F, ND), 3)
    K = F * D + ND
    arena = torch.zeros_like(inp["arena"])
    dense = [(torch.arange(B) % 16 == j).float() for j in range(ND)]
    d = {"arena": arena.to(DEV), "arena16": arena.to(torch.bfloat16).to(DEV),
         "rb": torch.tensor(inp["base"], dtype=torch.int64, device=DEV),
         "rc": torch.tensor(inp["rows"], dtype=torch.int64, device=DEV),
         "idx": [t.to(DEV) for t in inp["idx"]], "dense": [t.to(DEV) for t in dense], "K": K}
    worst, exact = 0.0, True
    for sign in (1.0, -1.0):
        W = inp["W"] * sign
        d["W"] = W.to(DEV)
        ref = first_layer_f64(arena.double(), inp["base"], inp["rows"], inp["idx"], dense, W, None)
        assert torch.equal(ref["pre"], W[:, F * D + torch.arange(B) % 16].T.double())
        out = run_wrapper(hip, d, form, round_up(K, 64), biased=False)
        assert int(out[5][0]) == 0
        h1 = out[1].double().cpu()
        bar = 2.0 ** -22 * ref["pre"].abs()
        assert bool(((h1 - ref["h1"]).abs() <= bar).all()), float(((h1 - ref["h1"]).abs() / bar.clamp_min(1e-30)).max())
        worst = max(worst, float(((h1 - ref["h1"]).abs() / bar.clamp_min(1e-30)).max()))
        exact = exact and torch.equal(h1, ref["h1"])
        assert not bool(out[2].any()), "fm of all-zero rows"
    print(f"\ndense k-step, {form}: worst share of 2^-22 |w| {worst:.3f}" + (" (bit-exact)" if exact else ""), end="")


# ---- the direct C call: the test owns every buffer ------------------------------------------------------------------------
def ptr(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def c_call(hip, d, bf16_rows, B, *, arena, W, ldw, bias, h1, fm, x, ldx, ssum, keys, err, xd, idx=None, dense=None, F=None, ND=None):
    idx, dense = idx or d["idx"], d["dense"] if dense is None else dense
    F, ND = len(idx) if F is None else F, len(dense) if ND is None else ND
    head = (ptr(arena), d["rb"].data_ptr(), d["rc"].data_ptr(), hip._ptr_array(idx), F, hip._ptr_array(dense), ND, B, D)
    if bf16_rows:
        return hip.lib().rp_embed_gather_linear_fwd_bf16(*head, ptr(W), ldw, ptr(bias), ptr(h1), ptr(fm), ptr(x), ldx, ptr(ssum),
                                                         ptr(keys), ptr(err), ptr(xd), hip._stream())
    return hip.lib().rp_embed_gather_linear_fwd(*head, ptr(x), ldx, ptr(W), ldw, ptr(bias), ptr(h1), ptr(fm), ptr(ssum), ptr(keys),
                                                ptr(err), ptr(xd), hip._stream())


def guarded(B, cols, dtype=torch.float32):
    """[B + 128, cols] (cols = 0: [B + 128]): the live rows NaN (int32: -1, never a key), the 128 behind them a sentinel"""
    shape = (B + GUARD_ROWS, cols) if cols else (B + GUARD_ROWS,)
    if dtype == torch.int32:
        buf = torch.full(shape, CANARY_I32, dtype=dtype, device=DEV)
        buf[:B] = -1
    elif dtype == torch.bfloat16:
        buf = torch.full(shape, CANARY_I16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        buf[:B] = float("nan")
    else:
        buf = torch.full(shape, CANARY_F32, dtype=dtype, device=DEV)
        buf[:B] = float("nan")
    return buf


def guard_intact(buf, B):
    tail = bits(buf[B:])
    want = {torch.int32: CANARY_I32, torch.bfloat16: CANARY_I16}.get(
        buf.dtype, torch.tensor(CANARY_F32, dtype=torch.float32).view(torch.int32).item())
    return tail.numel() == GUARD_ROWS * (buf.shape[1] if buf.dim() == 2 else 1) and bool((tail == want).all())


def owned_outputs(case, form, ldx):
    """every output buffer the form takes, with its guard; keys_out: F B entries + 128"""
    B, F, ND = case
    o = {"h1": guarded(B, 64), "fm": guarded(B, 0), "x": None, "xd": None, "ssum": None, "keys": None}
    if form == "full":
        o["x"] = guarded(B, ldx)
    if form == "x16":
        o["x"] = guarded(B, ldx, torch.bfloat16)
    if form in ("dense", "xd"):
        o["xd"] = guarded(B, 64)
    if form not in ("none", "infer"):
        o["ssum"] = guarded(B, 64)
        o["keys"] = guarded(F * B, 0, torch.int32)
    return o


def poisoned_w(d, pad):
    """W [64, K] as a view (ldw floats per row) into a larger buffer: columns [K, ldw) of every row and the 64 floats behind
    the last row hold `pad`"""
    K, ldw = d["K"], d["ldw"]
    buf = torch.full((64 * ldw + 64,), pad, device=DEV)
    w = buf[:64 * ldw].view(64, ldw)
    w[:, :K] = d["W"]
    assert buf.data_ptr() % 16 == 0 and ldw > K
    return buf, w


@pytest.mark.parametrize("B", [129, 421])
@pytest.mark.parametrize("form", F32_FORMS + BF16_FORMS)
def test_poisoned_surroundings(hip, form, B):
    """F = 5, ND = 13 (K % 4 = 1: three padding columns per row of W).  NaN in every arena row no sample looks up (the 127
    clamped lanes of B = 129's tail workgroup must read real rows), NaN behind column K of every row of W and behind its
    last row; every output buffer has 128 sentinel rows behind row B - 1 and NaN in its live part."""
    case = (B, 5, 13)
    _, F, ND = case
    d = dev_case(case)
    bf16_rows = form in BF16_FORMS
    ref = case_reference(case, bf16_rows, True)
    ldx = round_up(d["K"], 4)
    unused = case_inputs(case)["unused"].to(DEV)
    arena = (d["arena16"] if bf16_rows else d["arena"]).clone()
    arena[unused] = float("nan")
    assert bool(unused.any()) and bool(torch.isnan(arena[-1]).all())
    results = []
    for pad in (float("nan"), 0.0):
        wbuf, w = poisoned_w(d, pad)
        o = owned_outputs(case, form, ldx)
        err = new_flag()
        n0 = hip.launch_count()
        rc = c_call(hip, d, bf16_rows, B, arena=arena, W=w, ldw=d["ldw"], bias=d["bias"], h1=o["h1"], fm=o["fm"], x=o["x"],
                    ldx=ldx if o["x"] is not None else 0, ssum=o["ssum"], keys=o["keys"], err=err, xd=o["xd"])
        assert rc == OK and hip.launch_count() - n0 == 1
        assert int(err[0]) == 0 and int(err[1]) == 0, "err_flag"
        for name, buf in o.items():
            if buf is None:
                continue
            n = F * B if name == "keys" else B
            assert guard_intact(buf, n), f"{name}: a row >= B was written"
            live = buf[:n]
            if name == "keys":
                assert not bool((live == -1).any()), "keys_out: a live entry was not written"
            else:
                assert bool(torch.isfinite(live.float()).all()), f"{name}: a live element was not written, or is not finite"
        out = (o["x"][:B] if o["x"] is not None else (o["xd"][:B] if o["xd"] is not None else None), o["h1"][:B], o["fm"][:B],
               None if o["ssum"] is None else o["ssum"][:B], None if o["keys"] is None else o["keys"][:F * B], err)
        worst = {}
        check_results(form, ref, out, worst)
        check_stored(case, d, form, ref, out[0], ldx)
        assert max(worst.values()) <= 1.0, worst
        results.append(out)
    assert same_bits(results[0][1], results[1][1]), "h1 changes with what lies behind column K of W"
    agree(results[0], run_wrapper(hip, d, form, ldx), "the poisoned and the clean surroundings")


@pytest.mark.parametrize("which", range(len(BAD_IDS)), ids=["f%d-b%d-%s" % b for b in BAD_IDS])
@pytest.mark.parametrize("form", F32_FORMS + BF16_FORMS)
def test_id_outside_its_table_sets_the_flag_and_reads_row_zero(hip, form, which):
    """an id equal to row_count[f] / an id of -1, in a full workgroup / in the tail of B = 421: flagged in every form, the
    sample's field reads as the table's row 0.  (An id outside its table in a clamped, absent lane cannot occur: those lanes
    re-read sample B - 1; the clean B = 129 batch below leaves the flag at 0.)"""
    d = dev_case(BAD_CASE)
    ldx = round_up(d["K"], 64)
    err = new_flag()
    out = run_wrapper(hip, d, form, ldx, idx=[t.to(DEV) for t in bad_ids(which)], err=err)
    assert int(err[0]) == 1, "an id outside its table did not raise the flag"
    ref = case_reference(BAD_CASE, form in BF16_FORMS, True, which)
    worst = {}
    check_results(form, ref, out, worst)
    check_stored(BAD_CASE, d, form, ref, out[0], ldx)
    assert max(worst.values()) <= 1.0, worst
    clean = dev_case((129, 5, 13))
    assert int(run_wrapper(hip, clean, form, round_up(clean["K"], 64))[5][0]) == 0


def _refusal_case(F, ND):
    """a 5-sample batch on the device with its own tables (F may exceed what the launch takes)"""
    inp = first_layer_inputs((5, F, ND), 1)
    K = F * D + ND
    return {"arena": inp["arena"].to(DEV), "arena16": inp["arena"].to(torch.bfloat16).to(DEV),
            "rb": torch.tensor(inp["base"], dtype=torch.int64, device=DEV),
            "rc": torch.tensor(inp["rows"], dtype=torch.int64, device=DEV),
            "idx": [t.to(DEV) for t in inp["idx"]], "dense": [t.to(DEV) for t in inp["dense"]], "K": K,
            "bias": inp["bias"].to(DEV), "Wflat": torch.randn(64 * (K + 8) + 8, device=DEV)}


REFUSALS = {  # clause -> (F, ND, bf16 rows, ldw - K, W offset in floats, x, xd, ldx - K, x offset in elements, code)
    "F=33": (33, 0, False, 0, 0, False, False, 0, 0, ERR_UNSUPPORTED),
    "F=33-bf16": (33, 0, True, 0, 0, False, False, 0, 0, ERR_UNSUPPORTED),
    "ND=17": (2, 17, False, 3, 0, False, False, 0, 0, ERR_UNSUPPORTED),
    "ldw%4": (2, 13, False, 0, 0, False, False, 0, 0, ERR_UNSUPPORTED),
    "ldw%4-bf16": (2, 13, True, 1, 0, False, False, 0, 0, ERR_UNSUPPORTED),
    "W-unaligned": (2, 13, False, 3, 1, False, False, 0, 0, ERR_UNSUPPORTED),
    "W-unaligned-bf16": (2, 13, True, 3, 2, False, False, 0, 0, ERR_UNSUPPORTED),
    # the two below are contradictory / misaligned ARGUMENTS, not shapes no kernel was built for: the entry points answer
    # RP_ERR_ARG (rec_pangu_hip.h: "bad size / alignment / null pointer"), which hip.py's wrappers raise on like any other code
    "x-and-xd": (2, 13, False, 3, 0, True, True, 3, 0, ERR_ARG),
    "x-and-xd-bf16": (2, 13, True, 3, 0, True, True, 3, 0, ERR_ARG),
    "x_bf16-ldx%4": (2, 13, True, 3, 0, True, False, 1, 0, ERR_ARG),
    "x_bf16-2-bytes-off": (2, 13, True, 3, 0, True, False, 3, 1, ERR_ARG),
}


@pytest.mark.parametrize("clause", sorted(REFUSALS))
def test_refusals_issue_no_launch(hip, clause):
    F, ND, bf16_rows, w_pad, w_off, with_x, with_xd, x_pad, x_off, code = REFUSALS[clause]
    B = 5
    d = _refusal_case(F, ND)
    K = d["K"]
    ldw, ldx = K + w_pad, K + x_pad
    W = d["Wflat"][w_off:]
    assert W.data_ptr() % 16 == 4 * w_off
    xbuf = torch.full((B * (K + 8) + 8,), float("nan"), dtype=torch.bfloat16 if bf16_rows else torch.float32, device=DEV)
    x = xbuf[x_off:] if with_x else None
    assert x is None or x.data_ptr() % 16 == x_off * xbuf.element_size()
    xd = torch.full((B, 64), float("nan"), device=DEV) if with_xd else None
    h1, fm, ssum = (torch.full(s, float("nan"), device=DEV) for s in ((B, 64), (B,), (B, 64)))
    err = new_flag()

    def call(**changed):
        args = dict(arena=d["arena16"] if bf16_rows else d["arena"], W=W, ldw=ldw, bias=d["bias"], h1=h1, fm=fm, x=x,
                    ldx=ldx if with_x else 0, ssum=ssum, keys=None, err=err, xd=xd)
        args.update(changed)
        return c_call(hip, d, bf16_rows, B, **args)

    n0 = hip.launch_count()
    rc = call()
    torch.cuda.synchronize()
    assert rc == code, (clause, rc, hip.lib().rp_last_error())
    with pytest.raises(RuntimeError):
        hip._check(rc, clause)  # (what the wrappers do with the code)
    assert hip.launch_count() == n0, "a refused call launched"
    for t in (h1, fm, ssum, xbuf, xd):
        assert t is None or bool(torch.isnan(t.float()).all()), "a refused call wrote"
    assert int(err[0]) == 0


def test_wrappers_refuse_and_an_empty_batch_is_served_without_a_launch(hip):
    d = _refusal_case(2, 13)
    K, B = d["K"], 5
    W = d["Wflat"][:64 * (K + 3)].view(64, K + 3)[:, :K]
    n0 = hip.launch_count()
    assert not hip.embed_gather_linear_fits(D, 33, 0, 64, 33 * 64, torch.zeros(64, 33 * 64, device=DEV))
    assert not hip.embed_gather_linear_fits(D, 2, 17, 64, round_up(K + 4, 64), W)
    assert not hip.embed_gather_linear_fits(D, 2, 13, 64, round_up(K, 64), d["Wflat"][:64 * K].view(64, K))  # ldw % 4
    assert not hip.embed_gather_linear_fits(D, 2, 13, 64, round_up(K, 64), d["Wflat"][1:64 * (K + 3) + 1].view(64, K + 3)[:, :K])
    assert hip.embed_gather_linear_fits(D, 2, 13, 64, round_up(K, 64), W)
    with pytest.raises(RuntimeError):  # x_bf16 with ldx % 4 != 0
        hip.embed_gather_linear_fwd_bf16(d["arena16"], d["rb"], d["rc"], d["idx"], d["dense"], W, d["bias"], new_flag(), train_ldx=K)
    with pytest.raises(RuntimeError):  # ldw % 4 != 0
        hip.embed_gather_linear_fwd(d["arena"], d["rb"], d["rc"], d["idx"], d["dense"], round_up(K, 64),
                                    d["Wflat"][:64 * K].view(64, K), d["bias"], True, True, True, new_flag())
    assert hip.launch_count() == n0
    # B = 0: RP_OK, nothing launched, nothing written
    h1, fm = torch.full((B, 64), float("nan"), device=DEV), torch.full((B,), float("nan"), device=DEV)
    err = new_flag()
    for bf16_rows in (False, True):
        rc = c_call(hip, d, bf16_rows, 0, arena=d["arena16"] if bf16_rows else d["arena"], W=W, ldw=K + 3, bias=d["bias"], h1=h1,
                    fm=fm, x=None, ldx=0, ssum=None, keys=None, err=err, xd=None)
        torch.cuda.synchronize()
        assert rc == OK and hip.launch_count() == n0
    assert bool(torch.isnan(h1).all()) and bool(torch.isnan(fm).all()) and int(err[0]) == 0
    # and the same call with B = 5 is served
    assert c_call(hip, d, False, B, arena=d["arena"], W=W, ldw=K + 3, bias=d["bias"], h1=h1, fm=fm, x=None, ldx=0, ssum=None,
                  keys=None, err=err, xd=None) == OK
    assert hip.launch_count() == n0 + 1 and not bool(torch.isnan(h1).any()) and int(err[0]) == 0
