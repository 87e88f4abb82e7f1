"""The first layer's backward on the embedding columns (rp_embed_grad_reduce / _gemm / _seg / _ss / _smp / _tiny: the lookup's
backward + the FM term's + the first Linear's dgrad and the embedding columns of its weight gradient) stated once in
float64, and that statement proved on the host.  tests/test_hip_first_layer_backward_forms.py compares every launch family
with first_layer_backward_f64 over the inputs backward_inputs builds; this file checks, without a GPU,

  * the statement (the per-run formulas of include/rec_pangu_hip.h for rp_embed_grad_seg) against torch autograd in float64
    of the reference ops themselves: the gather, oracle.ref_ops.fm_second_order, torch.nn.functional.linear, with ssum = the
    sum of the gathered rows; and, with a FREE ssum (the kernels' contract allows any [B, 64]), against the per-pair
    formula of rp_embed_grad_reduce in float64,
  * the inputs: every table's first and last row looked up, a row per table nobody looks up (tables of >= 3 rows), the forced
    runs where the case asks for them, about 40 % exact zeros in dh,
  * the EXACT variant of the inputs (small integers): every sum a kernel can form, in any order, stays below 2^23 in
    magnitude (2^24 without the accumulate mode's 0.5), one operand of every matrix product fits 8 significant bits and the
    other 16 (the split-bf16 products drop nothing), and a float32 evaluation in a shuffled order equals the float64 one bit
    for bit — so torch.equal is a fair demand on the device,
  * the expected index work as plain host functions (the stable sort, rp_embed_grad_ss_mark's and rp_embed_grad_smp_mark's
    lists) on hand-made lists.

Bar (from test_hip_kernels.py, not loosened): per tensor max|got - ref| <= 2e-5 max(max|ref - init|, 1e-6)."""
import collections
import functools

import pytest
import torch

from oracle import ref_ops as R

torch.set_num_threads(1)

D = H = 64
ND = 5            # dense columns behind the embedding columns of W1: K = F 64 + ND (never read by these launches)
SPARE_ROWS = 2    # arena rows behind the last table (the GPU file's canary rows)
NEVER = 7.25      # what the GPU file keeps in the gradient rows nobody looked up

# spec: ((field, kind, arg), ...).  kind "runs": arg = ((row, length), ...) — exactly `length` samples look up `row`, nobody
# else does; "distinct": no two samples share a row; "pairs": every sample shares its row with another; default: random ids
Case = collections.namedtuple("Case", "tables B with_fm accumulate spec")


def case(tables, B, with_fm=True, accumulate=False, spec=()):
    return Case(tuple(tables), B, with_fm, accumulate, tuple(spec))


def _ids(r, B, g, kind, arg):
    """ids of one field -> (ids [B] int64 in shuffled sample order, the row nobody looks up or None)"""
    forced = {row: n for row, n in arg} if kind == "runs" else {}
    n_forced = sum(forced.values())
    assert n_forced <= B and all(0 <= row < r for row in forced)
    free = B - n_forced
    if kind == "distinct":
        assert r >= B + 1
        t = (torch.randperm(r - 2, generator=g)[:B] + 1) if B > 2 else torch.zeros(B, dtype=torch.int64)
        never = next(x for x in range(1, r) if x not in set(t.tolist()) and x != r - 1) if r >= B + 3 else None
        if B >= 2:
            t[0] = 0
        t[B - 1] = r - 1
        return t, never
    if kind == "pairs":
        assert B >= 2 and r >= 3
        t = torch.arange(B) // 2 % (r - 2)
        t = torch.where(t > 0, t + 1, t)  # row 1 is nobody's
        if B % 2:
            t[B - 1] = t[B - 2]
        last = t == t[B - 1]
        t[last] = r - 1
        return t[torch.randperm(B, generator=g)], 1
    candidates = [x for x in range(r) if x not in forced]
    never = None
    if len(candidates) >= 3 or (len(candidates) >= 1 and r >= 3 and free == 0):
        never = candidates[len(candidates) // 2]
    pool = torch.tensor([x for x in candidates if x != never], dtype=torch.int64)
    parts = [torch.full((n,), row, dtype=torch.int64) for row, n in forced.items()]
    if free:
        assert pool.numel() >= 1, "samples left, but every row is forced or kept free"
        t = pool[torch.randint(0, pool.numel(), (free,), generator=g)]
        if free >= 2 and 0 not in forced and never != 0:
            t[0] = 0
        if r - 1 not in forced:
            t[free - 1] = r - 1
        parts.append(t)
    t = torch.cat(parts)
    return t[torch.randperm(B, generator=g)], never


def backward_inputs(c, seed, exact=False):
    """the inputs of one case: tables back to back in one arena [sum rows + SPARE_ROWS, 64], F index tensors, dh [B, 64] with
    about 40 % exact zeros, W1 [64, F 64 + ND], gfm [B] and a FREE ssum [B, 64] (with_fm), `unused` = the mask of the arena
    rows nobody looks up, `never` = one such row per table (or None).  exact: dh, W1, gfm integers in -2..2, arena and ssum in -8..8."""
    g = torch.Generator().manual_seed(seed)
    F, B = len(c.tables), c.B
    rows = list(c.tables)
    base = [sum(rows[:f]) for f in range(F)]
    NR = sum(rows) + SPARE_ROWS
    K = F * D + ND
    spec = {f: (kind, arg) for f, kind, arg in c.spec}
    idx, never = [], []
    for f, r in enumerate(rows):
        t, nv = _ids(r, B, g, *spec.get(f, ("rand", ())))
        idx.append(t)
        never.append(None if nv is None else base[f] + nv)
    keep = torch.rand(B, H, generator=g) < 0.6
    if exact:
        ints = lambda shape, hi: torch.randint(-hi, hi + 1, shape, generator=g).float()  # noqa: E731
        arena, W1 = ints((NR, D), 8), ints((H, K), 2)
        dh = torch.randint(1, 3, (B, H), generator=g).float() * (2 * torch.randint(0, 2, (B, H), generator=g) - 1) * keep
        gfm, ssum = (ints((B,), 2), ints((B, D), 8)) if c.with_fm else (None, None)
    else:
        arena = torch.randn(NR, D, generator=g) * 0.3
        W1 = torch.randn(H, K, generator=g) / K ** 0.5
        dh = torch.randn(B, H, generator=g) * 1e-3 * keep
        gfm, ssum = (torch.randn(B, generator=g) * 1e-3, torch.randn(B, D, generator=g)) if c.with_fm else (None, None)
    unused = torch.ones(NR, dtype=torch.bool)
    for f in range(F):
        unused[base[f] + idx[f]] = False
    return {"rows": rows, "base": base, "arena": arena, "idx": idx, "dh": dh, "W1": W1, "gfm": gfm, "ssum": ssum,
            "unused": unused, "never": never, "init": 0.5 if c.accumulate else 0.0,
            "keys": torch.cat([base[f] + idx[f] for f in range(F)]).to(torch.int32)}


def first_layer_backward_f64(arena, base, rows, idx, dh, W1, gfm=None, ssum=None, init=0.0):
    """THE statement, per run of equal keys as rec_pangu_hip.h writes it for rp_embed_grad_seg: for the pairs (f, b) of table
    row r,  Hs = sum dh[b, :], u = sum gfm[b] ssum[b, :], s = sum gfm[b];
        G[r, :] = init + Hs . W1[:, f 64:(f + 1) 64] + u - s arena[r, :]        rows nobody looked up stay at init
        dw[:, f 64:(f + 1) 64] = sum over the field's runs of Hs^T (x) arena[r, :]
    -> (G [arena rows, 64], dw [64, F 64]) in float64.  A row nobody looks up is not read (it may hold NaN)."""
    assert (gfm is None) == (ssum is None)
    F, NR = len(idx), arena.shape[0]
    A, Wd, dhd = arena.double(), W1.double(), dh.double()
    G = torch.full((NR, D), float(init), dtype=torch.float64)
    dw = torch.zeros(H, F * D, dtype=torch.float64)
    for f in range(F):
        assert int(idx[f].min()) >= 0 and int(idx[f].max()) < rows[f]
        Hs = torch.zeros(rows[f], H, dtype=torch.float64).index_add_(0, idx[f], dhd)
        looked = torch.zeros(rows[f], dtype=torch.bool)
        looked[idx[f]] = True
        v = A[base[f]:base[f] + rows[f]][looked]
        g_rows = Hs[looked] @ Wd[:, f * D:(f + 1) * D]
        if gfm is not None:
            u = torch.zeros(rows[f], D, dtype=torch.float64).index_add_(0, idx[f], gfm.double()[:, None] * ssum.double())
            s = torch.zeros(rows[f], dtype=torch.float64).index_add_(0, idx[f], gfm.double())
            g_rows = g_rows + u[looked] - s[looked][:, None] * v
        G[base[f] + torch.nonzero(looked).flatten()] += g_rows
        dw[:, f * D:(f + 1) * D] = Hs[looked].T @ v
    return G, dw


def per_pair_backward(inp, dtype=torch.float64, order=None):
    """rp_embed_grad_reduce's per-pair formula, evaluated pair by pair in `order` (a permutation of the F B pairs; None: list
    order) in `dtype`: G[key] += dh[b] . W1_f + gfm[b] (ssum[b] - arena[key]);  dw = dh^T x over the gathered rows"""
    F, B = len(inp["idx"]), inp["dh"].shape[0]
    A, W, dh = inp["arena"].to(dtype), inp["W1"].to(dtype), inp["dh"].to(dtype)
    keys = inp["keys"].long()
    smp = torch.arange(F * B) % B
    dX = (dh @ W[:, :F * D]).view(B, F, D).transpose(0, 1).reshape(F * B, D)  # pair f B + b
    if inp["gfm"] is not None:
        dX = dX + inp["gfm"].to(dtype)[smp][:, None] * (inp["ssum"].to(dtype)[smp] - A[keys])
    order = torch.arange(F * B) if order is None else order
    G = torch.full(A.shape, inp["init"], dtype=dtype).index_add_(0, keys[order], dX[order])
    sorder = torch.arange(B) if order is None else order[order < B]
    x = A[keys.view(F, B).T].reshape(B, F * D)
    return G, dh[sorder].T @ x[sorder]


def embed_grad_reduce_f64(arena, keys, B, Dd, dx, gfm, ssum, init):
    """rp_embed_grad_reduce as its header states it, any row width Dd: G[key] += dx[b, f Dd:(f + 1) Dd] + gfm[b] (ssum[b] -
    arena[key]) over the pairs (f, b); dx None: no such term; ssum None with gfm: only - gfm[b] arena[key] is applied"""
    A = arena.double()
    keys = keys.long()
    F = keys.numel() // B
    G = torch.full(A.shape, float(init), dtype=torch.float64)
    for f in range(F):
        key = keys[f * B:(f + 1) * B]
        c = torch.zeros(B, Dd, dtype=torch.float64) if dx is None else dx.double()[:, f * Dd:(f + 1) * Dd]
        if gfm is not None:
            c = c + gfm.double()[:, None] * ((0.0 if ssum is None else ssum.double()) - A[key])
        G.index_add_(0, key, c)
    return G


# ---- the expected index work ------------------------------------------------------------------------------------------------
def stable_sort(keys):
    """rp_sort_pairs_i32: (sorted keys, positions), equal keys in ascending position"""
    sk, sp = torch.sort(keys.long(), stable=True)
    return sk, sp


def ss_marks(sk, B, skip_fields):
    """rp_embed_grad_ss_mark over the sorted keys [F B] -> per kept field, in field order: (ustart = positions inside the field
    where a run starts, ukey = their keys), and offs [kept * nbk + 1]: the number of runs in front of each 256-block, counted
    through all kept fields, the total last.  Field r_'s lists stand at [r_ * B, r_ * B + len) of the device lists."""
    F, nbk = sk.numel() // B, (B + 255) // 256
    lists, offs, run = [], [], 0
    for f in range(F):
        if (skip_fields >> f) & 1:
            continue
        ks = sk[f * B:(f + 1) * B]
        start = torch.ones(B, dtype=torch.bool)
        start[1:] = ks[1:] != ks[:-1]
        xs = torch.nonzero(start).flatten()
        lists.append((xs, ks[xs]))
        per_blk = torch.zeros(nbk, dtype=torch.int64).index_add_(0, xs // 256, torch.ones_like(xs))
        offs.append(run + torch.cumsum(per_blk, 0) - per_blk)
        run += xs.numel()
    return lists, torch.cat(offs + [torch.tensor([run])])


def smp_marks(sk, sp, B, fields):
    """rp_embed_grad_smp_mark -> (dupq [n_fields B], dupkeys [n_fields B]): the pairs of runs of >= 2 numbered in sorted
    order, field by field; dupq[fi B + b] = that number or -1; dupkeys[c] = the key of pair c, -1 from their count on"""
    dupq = torch.full((len(fields) * B,), -1, dtype=torch.int64)
    dupk = torch.full((len(fields) * B,), -1, dtype=torch.int64)
    c0 = 0
    for fi, f in enumerate(fields):
        ks, ps = sk[f * B:(f + 1) * B], sp[f * B:(f + 1) * B]
        assert bool(((ps >= f * B) & (ps < (f + 1) * B)).all())
        dup = torch.zeros(B, dtype=torch.bool)
        dup[1:] |= ks[1:] == ks[:-1]
        dup[:-1] |= ks[:-1] == ks[1:]
        c = c0 + torch.cumsum(dup.long(), 0) - 1
        dupq[fi * B + (ps - f * B)] = torch.where(dup, c, torch.full_like(c, -1))
        dupk[c[dup]] = ks[dup]
        c0 += int(dup.sum())
    return dupq, dupk


# ---- the cases the host proofs run over (the GPU file adds its own, built by the same functions) ------------------------
HOST_CASES = {
    "small-mixed": case([8, 4, 51, 12, 3], 24),
    "B1": case([5, 300, 1], 1),
    "no-fm-acc": case([3, 40, 500, 7], 130, with_fm=False, accumulate=True),
    "runs-512-513": case([40, 9, 600], 1100, spec=((0, "runs", ((0, 512), (3, 513))), (1, "runs", ((2, 5), (3, 513))))),
    "one-run": case([1, 30, 2], 300, accumulate=True, spec=((1, "runs", ((7, 300),)),)),
    "distinct-pairs": case([400, 77], 65, spec=((0, "distinct", ()), (1, "pairs", ()))),
    "F33": case([3] * 33, 20),
}
EXACT_LIMIT_B = 12500  # no case of the GPU file is larger


@functools.lru_cache(maxsize=None)
def host_inputs(name, exact=False):
    return backward_inputs(HOST_CASES[name], 17 + len(name), exact)


def statement(inp):
    return first_layer_backward_f64(inp["arena"], inp["base"], inp["rows"], inp["idx"], inp["dh"], inp["W1"], inp["gfm"],
                                    inp["ssum"], inp["init"])


def exactness_bounds(inp):
    """what makes an exact case exact, from the inputs alone -> (largest sum of magnitudes a gradient row / a dw element can
    see, largest |sum of dh| over any set of samples)"""
    F, B = len(inp["idx"]), inp["dh"].shape[0]
    for name in ("arena", "W1", "dh", "gfm", "ssum"):
        t = inp[name]
        if t is not None:
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= (8 if name in ("arena", "ssum") else 2), name
    absin = dict(inp, arena=inp["arena"].abs(), W1=inp["W1"].abs(), dh=inp["dh"].abs(), init=0.0,
                 gfm=None if inp["gfm"] is None else -inp["gfm"].abs(),
                 ssum=None if inp["ssum"] is None else -inp["ssum"].abs())  # -|gfm| (-|ssum| - |arena|): the magnitudes add
    Gabs, dwabs = per_pair_backward(absin)
    return max(float(Gabs.abs().max()), float(dwabs.abs().max())), float(inp["dh"].abs().sum(dim=0).max())


def assert_exact(inp):
    big, hs = exactness_bounds(inp)
    assert big + 1 < 2 ** 23, "a sum could leave the integers (and halves) float32 holds exactly"
    # matrix products: (sums of dh | arena | dh) x (W1 | sums of dh | arena): one side <= 8 significant bits, the other <= 16
    narrow = [inp["W1"], inp["arena"], inp["dh"]] + ([] if inp["gfm"] is None else [inp["gfm"], inp["gfm"][:, None] * inp["ssum"]])
    assert hs < 2 ** 16 and all(float(t.abs().max()) < 2 ** 8 for t in narrow)


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_inputs_reach_every_table_edge(name):
    c = HOST_CASES[name]
    for exact in (False, True):
        inp = host_inputs(name, exact)
        again = backward_inputs(c, 17 + len(name), exact)
        assert torch.equal(inp["arena"], again["arena"]) and torch.equal(inp["keys"], again["keys"])
        assert bool(inp["unused"][-SPARE_ROWS:].all())
        for f, r in enumerate(c.tables):
            t = inp["idx"][f]
            assert t.dtype == torch.int64 and t.shape == (c.B,) and int(t.min()) >= 0 and int(t.max()) < r
            whole = any(ff == f and kind == "runs" and sum(n for _, n in arg) == c.B for ff, kind, arg in c.spec)
            # (a field whose forced runs take the whole batch looks up those rows only)
            assert whole or (bool((t == r - 1).any()) and (c.B == 1 or bool((t == 0).any()))), (name, f)
            if r >= 3:
                nv = inp["never"][f]
                assert nv is not None and bool(inp["unused"][nv]) and inp["base"][f] <= nv < inp["base"][f] + r, (name, f)
        for f, kind, arg in c.spec:
            counts = torch.bincount(inp["idx"][f], minlength=c.tables[f])
            if kind == "runs":
                assert all(int(counts[row]) == n for row, n in arg)
            elif kind == "distinct":
                assert int(counts.max()) == 1
            else:
                assert int(counts[counts > 0].min()) >= 2
        zeros = float((inp["dh"] == 0).float().mean())
        assert c.B < 100 or 0.35 <= zeros <= 0.45, zeros


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_statement_against_autograd_of_the_reference_ops(name):
    inp = host_inputs(name)
    F, B = len(inp["idx"]), inp["dh"].shape[0]
    g = torch.Generator().manual_seed(5)
    A = inp["arena"].double().requires_grad_(True)
    W = inp["W1"].double().requires_grad_(True)
    dense = torch.rand(B, ND, generator=g).double()
    emb = A[inp["keys"].long().view(F, B).T]                       # the gather: [B, F, 64]
    pre = torch.nn.functional.linear(torch.cat([emb.reshape(B, F * D), dense], dim=1), W)
    loss = (pre * inp["dh"].double()).sum()
    ssum = None
    if inp["gfm"] is not None:
        loss = loss + (R.fm_second_order(emb)[:, 0] * inp["gfm"].double()).sum()
        ssum = emb.detach().sum(dim=1)
    loss.backward()
    G, dw = first_layer_backward_f64(inp["arena"], inp["base"], inp["rows"], inp["idx"], inp["dh"], inp["W1"], inp["gfm"], ssum, 0.0)
    gs, ws = float(A.grad.abs().max()), float(W.grad[:, :F * D].abs().max())
    assert float((G - A.grad).abs().max()) <= 1e-12 * gs and float((dw - W.grad[:, :F * D]).abs().max()) <= 1e-12 * ws
    assert not bool(G[inp["unused"]].any())


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_statement_with_a_free_ssum_against_the_per_pair_formula(name):
    inp = host_inputs(name)
    G, dw = statement(inp)
    Gp, dwp = per_pair_backward(inp)
    init = inp["init"]
    assert float((G - Gp).abs().max()) <= 1e-12 * float((Gp - init).abs().max())
    assert float((dw - dwp).abs().max()) <= 1e-12 * float(dwp.abs().max())
    assert bool((G[inp["unused"]] == init).all())
    F = len(inp["idx"])
    Gr = embed_grad_reduce_f64(inp["arena"], inp["keys"], inp["dh"].shape[0], D, inp["dh"].double() @ inp["W1"].double()[:, :F * D],
                               inp["gfm"], inp["ssum"], init)
    assert float((Gr - Gp).abs().max()) <= 1e-12 * float((Gp - init).abs().max())
    poisoned = dict(inp, arena=inp["arena"].masked_fill(inp["unused"][:, None], float("nan")))
    G2, dw2 = statement(poisoned)
    assert torch.equal(G2, G) and torch.equal(dw2, dw), "the statement read a row nobody looked up"


@pytest.mark.parametrize("name", sorted(HOST_CASES))
def test_exact_inputs_are_exact_in_float32_in_any_order(name):
    inp = host_inputs(name, True)
    assert_exact(inp)
    G, dw = statement(inp)
    F, B = len(inp["idx"]), inp["dh"].shape[0]
    for seed in (1, 2):
        order = torch.randperm(F * B, generator=torch.Generator().manual_seed(seed))
        G32, dw32 = per_pair_backward(inp, torch.float32, order)
        assert G32.dtype == torch.float32 and torch.equal(G32.double(), G) and torch.equal(dw32.double(), dw)
    assert torch.equal(G.float().double(), G) and torch.equal(dw.float().double(), dw)


def test_exactness_holds_at_the_largest_batch_the_gpu_file_uses():
    """the worst a case of EXACT_LIMIT_B samples can reach: every sample on one row, every value at its limit"""
    per_pair = H * 2 * 2 + 2 * (8 + 8)           # |dh| . |W1| over 64 hidden + |gfm| (|ssum| + |arena|)
    assert EXACT_LIMIT_B * per_pair + 1 < 2 ** 23
    assert EXACT_LIMIT_B * 2 < 2 ** 16           # a sum of dh over any samples fits 16 bits
    assert EXACT_LIMIT_B * 2 * 8 < 2 ** 23       # an element of dw


def test_expected_marks_on_hand_made_lists():
    B = 5
    keys = torch.tensor([3, 1, 3, 0, 3,   7, 9, 8, 6, 5,   10, 10, 11, 11, 12])  # fields of 4, 5 and 3 rows at 0, 5, 10
    sk, sp = stable_sort(keys)
    assert sk.tolist() == [0, 1, 3, 3, 3, 5, 6, 7, 8, 9, 10, 10, 11, 11, 12]
    assert sp.tolist() == [3, 1, 0, 2, 4, 9, 8, 5, 7, 6, 10, 11, 12, 13, 14]
    lists, offs = ss_marks(sk, B, 0b010)
    assert [x.tolist() for x, _ in lists] == [[0, 1, 2], [0, 2, 4]] and [k.tolist() for _, k in lists] == [[0, 1, 3], [10, 11, 12]]
    assert offs.tolist() == [0, 3, 6]
    dupq, dupk = smp_marks(sk, sp, B, [0, 2])
    assert dupq.tolist() == [0, -1, 1, -1, 2, 3, 4, 5, 6, -1] and dupk.tolist() == [3, 3, 3, 10, 10, 11, 11, -1, -1, -1]
    dupq, dupk = smp_marks(sk, sp, B, [1])
    assert dupq.tolist() == [-1] * 5 and dupk.tolist() == [-1] * 5
    # 256-blocks: runs that start in the second block are counted there
    keys = torch.cat([torch.zeros(255, dtype=torch.int64), torch.arange(1, 4)])
    lists, offs = ss_marks(*stable_sort(keys)[:1], 258, 0)
    assert lists[0][0].tolist() == [0, 255, 256, 257] and offs.tolist() == [0, 2, 4]
