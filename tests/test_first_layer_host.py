"""The fused first layer (rp_embed_gather_linear_fwd: lookup + concat + FM second order + the 64-wide Linear + ReLU) stated
once in float64, and that statement proved on the host.  tests/test_hip_first_layer_forms.py compares every form of the
kernel with first_layer_f64 over the inputs first_layer_inputs builds; this file checks, without a GPU,

  * the statement against the project's oracle in fp32 (oracle.ref_ops.fm_second_order, torch.nn.functional.linear + relu
    over the concatenated rows) at the GPU file's own bars,
  * the bf16 expectation of the stored dense columns: torch's float32 -> bfloat16 conversion is round-to-nearest-even on the
    32-bit pattern, bit for bit (ties both ways, +-0, a subnormal, values just below a power of two; no NaN / inf — the
    kernel's add-and-shift rounding is not specified for them),
  * the condition of the tight h1 bar.  A pre-activation within rounding of zero may land on either side of the ReLU, so
    |h1 - relu(pre)| <= 2e-5 max|pre| is asserted only where |pre| > 1e-5 max|pre| (4e-5 max|pre| holds everywhere).  The
    share of entries NOT clear of zero is at most 1e-3 in every reference the GPU file uses (every case, fp32 and
    bf16-rounded tables, with and without bias, the repaired-id references of the error-flag test): decided here, from the
    float64 reference alone.  For roughly Gaussian pre-activations the expected share is a few 1e-5.

Bars (from test_embed_gather_linear_vs_unfused, not loosened): h1 as above; ssum rtol = atol = 1e-5;
|fm - ref| <= 1e-6 (sum |emb|)^2 + 1e-5."""
import functools
import struct

import pytest
import torch

from oracle import ref_ops as R

torch.set_num_threads(1)

D = H = 64
TABLE_SIZES = (300, 1, 5000, 2, 7, 3)
# (B, F, ND).  B: 1 / 37 / 127 only the masked tail launch, 128 / 256 only the full launch, 129 a tail with one live sample,
# 421 three full workgroups + a 37-sample tail.  F: 1 (the prefetch re-reads field 0), 2 (one field per k-half of the key
# fill), 5 (odd), 26 (Criteo), 32 (the limit).  ND: 0 (no dense branch), 8 | 9 (either side of the k-half split), 13
# (Criteo; K % 4 != 0, as with 1 and 9), 16 (the limit).  Every B meets ND = 0 and an ND > 8.
CASES = [(1, 1, 0), (1, 5, 13), (1, 32, 16), (1, 2, 1),
         (37, 2, 0), (37, 26, 13), (37, 5, 9), (37, 1, 8),
         (127, 5, 0), (127, 32, 16), (127, 1, 1), (127, 2, 9),
         (128, 26, 0), (128, 2, 9), (128, 5, 8), (128, 1, 16),
         (129, 1, 0), (129, 5, 13), (129, 32, 1), (129, 26, 8), (129, 2, 16),
         (256, 32, 0), (256, 1, 13), (256, 2, 8), (256, 5, 16),
         (421, 2, 0), (421, 5, 13), (421, 26, 13), (421, 32, 9), (421, 1, 1), (421, 26, 16)]
SEEDS = {}  # case -> seed, where the default (below) leaves too many pre-activations within rounding of zero
NOT_CLEAR_SHARE = 1e-3
# the error-flag test: (field, sample, "past" = row_count[f] | "neg" = -1) in the case below — a full workgroup and the tail
BAD_CASE = (421, 5, 13)
BAD_IDS = [(1, 10, "past"), (3, 200, "neg"), (0, 400, "past"), (4, 420, "neg")]


def case_seed(case):
    B, F, ND = case
    return SEEDS.get(case, 1000 * B + 10 * F + ND)


def first_layer_inputs(case, seed):
    """the inputs of one (B, F, ND) case: tables of TABLE_SIZES rows back to back in one arena [sum rows + 1, 64] (the
    project's arenas end in one spare row), F index tensors, ND dense columns, W [64, K], bias [64], and `unused`, the
    boolean mask of the arena rows no sample looks up.  Every table's first and last row is looked up at least once (B = 1:
    the last row only) and, from B = 4 on, two samples of every field share an id."""
    B, F, ND = case
    g = torch.Generator().manual_seed(seed)
    off = 0 if F < 3 else (B + ND) % len(TABLE_SIZES)
    rows = [TABLE_SIZES[(f + off) % len(TABLE_SIZES)] for f in range(F)]
    base = [sum(rows[:f]) for f in range(F)]
    arena = torch.randn(sum(rows) + 1, D, generator=g) * 0.3
    idx = []
    for f, r in enumerate(rows):
        t = torch.randint(0, r, (B,), generator=g)
        if B >= 4:
            t[(3 * f + 3) % B] = t[(3 * f + 2) % B]
        if B >= 2:
            t[(3 * f) % B] = 0
        t[(3 * f + 1) % B] = r - 1
        idx.append(t)
    dense = [torch.rand(B, generator=g) for _ in range(ND)]
    K = F * D + ND
    W = torch.randn(H, K, generator=g) / K ** 0.5
    bias = torch.randn(H, generator=g) * 0.1
    unused = torch.ones(arena.shape[0], dtype=torch.bool)
    for f in range(F):
        unused[base[f] + idx[f]] = False
    return {"rows": rows, "base": base, "arena": arena, "idx": idx, "dense": dense, "W": W, "bias": bias, "unused": unused}


def first_layer_f64(arena, base, rows, idx, dense, W, bias):
    """THE statement.  arena: what the kernel reads, as float64 (bf16 forms: arena.to(torch.bfloat16) widened) -> float64
    pre [B, 64] = x W^T + bias, h1 = relu(pre), fm [B] = 0.5 sum_d ((sum_f v)^2 - sum_f v^2), ssum [B, 64] = sum_f v, the
    exact x [B, K] = (rows of the F fields | dense columns), and int32 keys [F B], keys[f B + b] = base[f] + idx[f][b]."""
    assert arena.dtype == torch.float64
    F, B = len(idx), idx[0].shape[0]
    for f in range(F):
        assert int(idx[f].min()) >= 0 and int(idx[f].max()) < rows[f], "the statement is for ids inside their tables"
    keys = torch.stack([base[f] + idx[f] for f in range(F)])
    emb = arena[keys.T]  # [B, F, 64]
    x = torch.cat([emb.reshape(B, F * D)] + [d.double()[:, None] for d in dense], dim=1)
    pre = x @ W.double().T
    if bias is not None:
        pre = pre + bias.double()
    ssum = emb.sum(dim=1)
    fm = 0.5 * (ssum * ssum - (emb * emb).sum(dim=1)).sum(dim=1)
    return {"pre": pre, "h1": pre.clamp_min(0), "fm": fm, "ssum": ssum, "keys": keys.reshape(-1).to(torch.int32), "x": x}


def table_f64(inp, bf16_rows):
    return (inp["arena"].to(torch.bfloat16) if bf16_rows else inp["arena"]).double()


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    return first_layer_inputs(case, case_seed(case))


@functools.lru_cache(maxsize=None)
def case_reference(case, bf16_rows=False, biased=True, repaired=None):
    """the float64 results of a case: computed once, shared, left unchanged.  repaired = i: BAD_IDS[i]'s id replaced by 0,
    what the kernel reads for an id outside its table"""
    inp = case_inputs(case)
    idx = inp["idx"]
    if repaired is not None:
        f, b, _ = BAD_IDS[repaired]
        idx = [t.clone() for t in idx]
        idx[f][b] = 0
    return first_layer_f64(table_f64(inp, bf16_rows), inp["base"], inp["rows"], idx, inp["dense"], inp["W"],
                           inp["bias"] if biased else None)


def bad_ids(i):
    """the index tensors of BAD_CASE with the one id BAD_IDS[i] outside its table"""
    inp = case_inputs(BAD_CASE)
    f, b, kind = BAD_IDS[i]
    idx = [t.clone() for t in inp["idx"]]
    idx[f][b] = inp["rows"][f] if kind == "past" else -1
    return idx


def h1_shares(h1, ref):
    """(worst error where |pre| is clear of zero / its bar 2e-5 max|pre|, worst error anywhere / 4e-5 max|pre|)"""
    pre = ref["pre"].to(h1.device)
    scale = float(pre.abs().max())
    err = (h1.double() - pre.clamp_min(0)).abs()
    clear = pre.abs() > 1e-5 * scale
    return float((err * clear).max()) / (2e-5 * scale), float(err.max()) / (4e-5 * scale)


def ssum_share(ssum, ref):
    want = ref["ssum"].to(ssum.device)
    return float(((ssum.double() - want).abs() / (1e-5 + 1e-5 * want.abs())).max())


def fm_share(fm, ref):
    F = ref["keys"].numel() // ref["x"].shape[0]
    want = ref["fm"].to(fm.device)
    bar = 1e-6 * ref["x"][:, :F * D].abs().sum(dim=1).to(fm.device) ** 2 + 1e-5
    return float(((fm.double().reshape(-1) - want).abs() / bar).max())


def all_references():
    for case in CASES:
        for bf16_rows in (False, True):
            for biased in (True, False):
                yield (case, bf16_rows, biased, None)
    for i in range(len(BAD_IDS)):
        for bf16_rows in (False, True):
            yield (BAD_CASE, bf16_rows, True, i)


def test_the_case_list_covers_what_it_claims():
    Bs, Fs, NDs = (1, 37, 127, 128, 129, 256, 421), (1, 2, 5, 26, 32), (0, 1, 8, 9, 13, 16)
    assert len(set(CASES)) == len(CASES) and 28 <= len(CASES) <= 34
    for pos, values in enumerate((Bs, Fs, NDs)):
        seen = [c[pos] for c in CASES]
        assert set(seen) == set(values)
        assert all(seen.count(v) >= 2 for v in values), (pos, seen)
    for B in Bs:
        nds = {nd for b, _, nd in CASES if b == B}
        assert 0 in nds and max(nds) > 8, B
    sizes = {r for c in CASES for r in case_inputs(c)["rows"]}
    assert sizes == set(TABLE_SIZES)
    assert BAD_CASE in CASES
    for f, b, kind in BAD_IDS:
        assert f < BAD_CASE[1] and b < BAD_CASE[0]
    assert {(b < 384, kind) for _, b, kind in BAD_IDS} == {(True, "past"), (True, "neg"), (False, "past"), (False, "neg")}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-F%d-ND%d" % c)
def test_inputs_reach_every_table_edge(case):
    B, F, ND = case
    inp = case_inputs(case)
    again = first_layer_inputs(case, case_seed(case))
    assert torch.equal(inp["arena"], again["arena"]) and all(torch.equal(a, b) for a, b in zip(inp["idx"], again["idx"]))
    assert len(inp["idx"]) == F and len(inp["dense"]) == ND and inp["W"].shape == (H, F * D + ND)
    assert inp["arena"].shape[0] == sum(inp["rows"]) + 1 and bool(inp["unused"][-1])
    used = torch.zeros_like(inp["unused"])
    for f, r in enumerate(inp["rows"]):
        t = inp["idx"][f]
        assert t.dtype == torch.int64 and int(t.min()) >= 0 and int(t.max()) < r
        assert bool((t == r - 1).any()) and (B == 1 or bool((t == 0).any()))
        assert B < 4 or t.unique().numel() < B, "no duplicate id"
        used[inp["base"][f] + t] = True
    assert torch.equal(inp["unused"], ~used)
    for b16 in (False, True):  # nothing the kernel reads is NaN / inf
        assert bool(torch.isfinite(table_f64(inp, b16)).all())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-F%d-ND%d" % c)
def test_statement_against_the_oracle_in_fp32(case):
    B, F, ND = case
    inp = case_inputs(case)
    emb = torch.stack([inp["arena"][inp["base"][f] + inp["idx"][f]] for f in range(F)], dim=1)  # [B, F, 64] fp32
    x = torch.cat([emb.reshape(B, F * D)] + [d[:, None] for d in inp["dense"]], dim=1)
    for biased in (True, False):
        ref = case_reference(case, False, biased)
        assert torch.equal(ref["x"], x.double()), "x is a copy"
        assert torch.equal(ref["keys"].view(F, B)[F - 1].long(), inp["base"][F - 1] + inp["idx"][F - 1])
        h1 = torch.relu(torch.nn.functional.linear(x, inp["W"], inp["bias"] if biased else None))
        clear, everywhere = h1_shares(h1, ref)
        assert clear <= 1.0 and everywhere <= 1.0, (clear, everywhere)
        assert fm_share(R.fm_second_order(emb), ref) <= 1.0
        assert ssum_share(emb.sum(dim=1), ref) <= 1.0
        assert torch.equal(ref["h1"], ref["pre"].clamp_min(0))


@pytest.mark.parametrize("ref_id", list(all_references()), ids=lambda r: "B%d-F%d-ND%d" % r[0] + ("-bf16" if r[1] else "-f32")
                         + ("" if r[2] else "-nobias") + ("" if r[3] is None else "-repaired%d" % r[3]))
def test_few_pre_activations_lie_within_rounding_of_zero(ref_id):
    pre = case_reference(*ref_id)["pre"]
    share = float((pre.abs() <= 1e-5 * float(pre.abs().max())).double().mean())
    assert share <= NOT_CLEAR_SHARE, f"{share:.2e} of the entries are left out of the tight h1 bar: choose another seed (SEEDS)"


def bf16_bits_rne(u32):
    """round-to-nearest-even of a float32 bit pattern to its upper 16 bits, in plain integers"""
    lower, upper = u32 & 0xFFFF, u32 >> 16
    if lower > 0x8000 or (lower == 0x8000 and upper & 1):
        upper += 1
    return upper & 0xFFFF


def test_dense_to_bfloat16_is_round_to_nearest_even_on_the_bits():
    g = torch.Generator().manual_seed(7)
    values = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),  # ties: down to even, up to even
              0.0, -0.0, -0.3, 1e-40, -1e-40, 2.0 ** -126 - 2.0 ** -149,  # +-0, a negative value, subnormals
              2 - 2.0 ** -23, 1 - 2.0 ** -24, 4 - 2.0 ** -21, 0.99999, -(8 - 2.0 ** -20),  # just below a power of two: carry into the exponent
              1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 1.0, 0.5, 3.3895314e38 / 2]
    t = torch.cat([torch.tensor(values, dtype=torch.float32), torch.rand(4096, generator=g),
                   torch.randn(4096, generator=g) * 1e3, torch.randn(1024, generator=g) * 1e-41])
    assert bool(torch.isfinite(t).all())
    assert struct.unpack("<I", struct.pack("<f", values[0]))[0] == 0x3F808000  # the tie is exact in fp32
    got = [v & 0xFFFF for v in t.to(torch.bfloat16).view(torch.int16).tolist()]
    want = [bf16_bits_rne(v & 0xFFFFFFFF) for v in t.view(torch.int32).tolist()]
    assert got == want
    assert got[0] == 0x3F80 and got[1] == 0x3F82 and got[2] == 0xBF80 and got[3] == 0xBF82 and got[4] == 0 and got[5] == 0x8000
    assert got[10] == 0x4000 and got[11] == 0x3F80  # 2 - 2^-23 -> 2, 1 - 2^-24 -> 1
    # the kernel's form of the same rounding: add 0x7FFF + the kept part's last bit, shift (finite values)
    assert want == [(((v & 0xFFFFFFFF) + 0x7FFF + (((v & 0xFFFFFFFF) >> 16) & 1)) >> 16) & 0xFFFF for v in t.view(torch.int32).tolist()]
