"""Every launch family of the first layer's backward (csrc/embed.hip, embed_ss.hip, embed_smp.hip, embed_tiny.hip) called
alone through the C ABI, and composed as production composes them, against first_layer_backward_f64, the float64 statement
of tests/test_first_layer_backward_host.py, over inputs that file's backward_inputs builds:

    rp_embed_grad_reduce / rp_embed_grad_gemm      B = 1 / 127 / 128 / 129, a run across three 128-position tiles, D = 1 / 40 /
                                                   64, dx with ldx != F D, sum_in = NULL with gfm, F = 64 with alternating
                                                   skip_fields (32 ranges, bits >= 32 set and clear)
    rp_embed_grad_seg                              runs cut at 8-position pieces and 128-row tiles, T = 1, T = 2 with a ragged
                                                   last chunk (tpf = 97), field_rows given / NULL / ties / both orders, F = 33
                                                   with only field 32 kept
    rp_embed_grad_ss (+ rp_embed_grad_ss_mark)     B = 31 .. 513, 128 / 129 unique rows, rows of 16 / 17 chunk pieces on and off
                                                   a 32-position border, one run = the field, marks ahead / inside, phases
    rp_embed_grad_smp (+ _mark, _reduce_rows)      B = 1 / 63 / 64 / 65, no duplicate, all duplicates, one run, 1 / 2 / 3 / 16
                                                   fields, nranges > 1 ragged, keys above 2^23, phases
    rp_embed_grad_tiny                             B = 1 .. 65, 8192 / 8193, 2 / 8 / 9 / 16 tables, 224 rows together, a 1-row
                                                   table, a 224-row table alone, fields not adjacent, with / without dw, lddh = 68
    tiny + smp + ss                                marks ahead, phases split, one G and one dw, both accumulate modes, vs _seg

rp_embed_grad_gemm is also run with dx [B, F 64 + 4] (its own per-pair read of dx, with and without skip_fields).

Around every call: the gradient arena has canary rows behind the last table, 7.25 in every row nobody looks up and NaN in
the rows of the fields the call leaves out; dw starts at NaN with canary columns behind F 64; the mark lists have canary
slots behind their documented sizes; the workspace is exactly what the *_workspace_bytes function asks for, filled with
0xFF (NaN / -1), with a guard region behind it; rows >= B of dh / ssum / gfm, columns >= 64 of a strided dh, columns >= F 64
and rows >= 64 of W1, rows >= F 64 of W1^T and every arena row nobody looks up hold NaN (and the same call over clean
surroundings gives the same bits); two launches give the same bits.  The float inputs are held to the project's bar for
these kernels (the last test checks that no launch wrote an input), max|got - ref| <= 2e-5 max(max|ref - init|, 1e-6) per tensor over what the call covers; the exact-integer
inputs to torch.equal with the float64 result (the host file proves that demand fair).  What a family refuses it refuses
with its documented code, without a launch and without a write.

Worst error as a share of the bar per form (printed per test and at the end of the module: run with -s), as observed on
the MI355X:
  reduce          G 0.064   (sum_in = NULL: 0.100; D = 1: 0.009; D = 40: 0.005)
  gemm            G 0.068   (with dx: 0.065; F = 64 with skip_fields: 0.018; F = 33, field 32 alone: 0.015; lddh = 68: 0.143)
  seg             G 0.089   dw 0.011   (F = 33, field 32 alone: 0.007 / 0.011; lddh = 68: 0.142 / 0.019)
  ss              G 0.132   dw 0.015   (F = 33: 0.007 / 0.009; lddh = 68: 0.142 / 0.023)
  smp             G 0.179   dw 0.009   (lddh = 68: 0.141 / 0.008)
  tiny            G 0.081   dw 0.035
  tiny + smp + ss G 0.021   dw 0.010
No form lands above a fifth of the bar; every exact-integer case gave the float64 result bit for bit in every form.
"""
import ctypes as C
import functools
import types
import zlib

import pytest
import torch

from conftest import require_gpu
from test_first_layer_backward_host import (D, H, ND, NEVER, SPARE_ROWS, EXACT_LIMIT_B, assert_exact, backward_inputs, case,
                                            embed_grad_reduce_f64, exactness_bounds, smp_marks, ss_marks, stable_sort, statement)

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3
CANARY_F32, CANARY_I32, GUARD_BYTES, GUARD_SLOTS, PAD_ROWS = -12345.6789, 0x5A5A5A5A, 4096, 64, 3
BIG_KEY = 9_000_000  # > 2^23: the first arena row of a case whose tables stand that far into an (imagined) arena
WORST = {}  # form -> tensor -> worst share of the bar
ALL_CTX = []  # every case uploaded so far


def uniq(rows, skip_row, B):
    """runs over every row of a table but skip_row: two samples each, the rest of the batch on the last one"""
    ids = [r for r in range(rows) if r != skip_row]
    assert B >= 2 * len(ids)
    return tuple((r, 2) for r in ids[:-1]) + ((ids[-1], B - 2 * (len(ids) - 1)),)


CASES = {
    # ---- rp_embed_grad_reduce / _gemm: tiles of 128 sorted positions
    "B1": case([5, 300, 3], 1), "B127": case([5, 300, 3], 127, accumulate=True), "B128": case([5, 300, 3], 128, with_fm=False),
    "B129": case([5, 300, 3], 129),
    # field 0: row 1's run stands at positions 120 .. 269 (tiles 0, 1, 2; cut at 8-position pieces as well); field 1: random
    "run-3-tiles": case([5, 600], 400, spec=((0, "runs", ((0, 120), (1, 150))),)),
    "F64": case([3] * 64, 20),
    # ---- rp_embed_grad_seg
    "small-T1": case([8, 4, 51, 12, 3], 24),
    "T2-ragged": case([20000, 50, 3], 12300),                 # tpf = 97 tiles, T = 2: 49 chunks per field, the last of one tile of 12 rows
    "rows-asc-ties": case([50, 50, 700, 20000], 300, accumulate=True), "rows-desc": case([20000, 700, 50, 50], 300, with_fm=False),
    "F33-last": case([3] * 32 + [40], 130),
    # ---- rp_embed_grad_ss: 32-position chunks, 256-position mark blocks, tiles of 128 unique rows
    **{"ss-B%d" % b: case([6, 200], b, accumulate=b % 2 == 0, with_fm=b != 255) for b in (31, 32, 33, 255, 256, 257, 511, 513)},
    "uniq-128": case([129, 9], 300, spec=((0, "runs", uniq(129, 127, 300)),)),
    "uniq-129": case([130, 9], 300, spec=((0, "runs", uniq(130, 64, 300)),)),
    # field 0: 512 on a border (16 pieces) then 513 on a border (17); field 1: 513 from position 5 (17); field 2: 480 from
    # position 5 (16 pieces); field 3: 512 from position 5 (17 pieces)
    "long-rows": case([40, 9, 600, 12], 1100, spec=((0, "runs", ((0, 512), (1, 513))), (1, "runs", ((0, 5), (1, 513))),
                                                    (2, "runs", ((0, 5), (1, 480))), (3, "runs", ((0, 5), (1, 512))))),
    "one-run": case([1, 30, 2], 300, accumulate=True, spec=((1, "runs", ((7, 300),)),)),
    # ---- rp_embed_grad_smp: units of 64 samples
    **{"smp-B%d" % b: case([20000, 300], b, accumulate=b == 64, with_fm=b != 63) for b in (1, 63, 64, 65)},
    "smp-distinct": case([400, 20000], 200, spec=((0, "distinct", ()), (1, "distinct", ()))),
    "smp-pairs": case([400, 77, 20000], 131, accumulate=True, spec=((0, "pairs", ()), (1, "pairs", ()), (2, "pairs", ()))),
    "smp-one-run": case([1, 20000, 77], 2053, spec=((1, "runs", ((11, 2053),)),)),
    "smp-16-fields": case([700, 30] * 8, 4100),                 # 65 blocks x 8 field groups: bpw = 2, 33 ranges, the last of one block
    # ---- rp_embed_grad_tiny: chunks of 64 samples, ~128 blocks of samples
    **{"tiny-B%d" % b: case([3, 500, 7], b, accumulate=b == 65, with_fm=b != 63) for b in (1, 63, 64, 65)},
    "tiny-B8192": case([25, 4, 1000, 28], 8192), "tiny-B8193": case([25, 4, 1000, 28], 8193, accumulate=True),  # per_blk 64 / 128
    "tiny-8": case([3, 40, 7, 11, 500, 100, 5, 2, 9], 300),
    "tiny-9": case([3, 40, 7, 11, 500, 30, 5, 2, 9, 13], 300, with_fm=False),
    "tiny-16-224": case([1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 4, 6, 8, 45], 700, accumulate=True),  # 224 rows together
    "tiny-224-alone": case([224, 300], 500),
    # ---- the composition: tiny 0, 2, 4 / sample-major 3, 6 / streaming segment sums 1, 5
    "mix": case([3, 500, 40, 20000, 7, 1000, 15000], 2053), "mix-acc": case([3, 500, 40, 20000, 7, 1000, 15000], 2053, accumulate=True),
    # ---- the refusals: tiny 0, 2 / sample-major 1, 3
    "refuse": case([5, 20000, 3, 700], 70),
}
assert max(c.B for c in CASES.values()) <= EXACT_LIMIT_B


@pytest.fixture(scope="module")
def hip():
    require_gpu()
    from rec_pangu_amd import hip as h
    h.lib()
    try:
        yield h
    finally:
        for form in sorted(WORST):
            print(f"\nworst share of bar, {form}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(WORST[form].items())), end="")
        print()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def round_up(n, m):
    return (n + m - 1) // m * m


def P(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def ctx(name, exact=False, lddh=64, poison=True, key_off=0):
    """a case on the device, uploaded once, shared, left unchanged (the last test of the file compares every input buffer with
    the copy taken here): the inputs inside their poisoned (poison = False: zeroed) surroundings, the host-sorted pair list,
    the float64 results.  key_off: every key is raised by it and the arena / gradient arena pointers are lowered by as many
    rows, so that the same small buffers stand at rows >= key_off of a huge arena.  ONLY for rp_embed_grad_smp (run_family
    refuses it elsewhere): that launch addresses every row as its table's base + the row inside the table, idle lanes
    included (they read the table's row 0), so every address lies inside the buffers.  A launch that reads arena row 0 for
    an idle lane, as rp_embed_grad_ss does, would read 2.3 GB in front of the allocation: a device fault on a shared machine,
    not a failed assertion.  Whoever changes rp_embed_grad_smp's addressing re-reads it before running these two cases."""
    c = CASES[name]
    inp = backward_inputs(c, zlib.crc32(name.encode()) % 100000, exact)
    if exact:
        assert_exact(inp)
    Gref, dwref = statement(inp)
    F, B = len(c.tables), c.B
    K = F * D + ND
    pad = float("nan") if poison else 0.0
    d = types.SimpleNamespace(name=name, case=c, inp=inp, exact=exact, F=F, B=B, K=K, NR=inp["arena"].shape[0], init=inp["init"],
                              acc=c.accumulate, key_off=key_off, lddh=lddh, ldw=round_up(K, 4) + 4, lddw=F * D + 8)
    arena = inp["arena"].clone()
    arena[inp["unused"]] = pad
    d.arena = arena.to(DEV)
    d.dhbuf = torch.full((B + PAD_ROWS, lddh), pad, device=DEV)
    d.dhbuf[:B, :H] = inp["dh"].to(DEV)
    d.gfm = d.ssum = None
    if c.with_fm:
        d.ssum = torch.full((B + PAD_ROWS, D), pad, device=DEV)
        d.ssum[:B] = inp["ssum"].to(DEV)
        d.gfm = torch.full((B + PAD_ROWS,), pad, device=DEV)
        d.gfm[:B] = inp["gfm"].to(DEV)
    d.w = torch.full((H + 2, d.ldw), pad, device=DEV)
    d.w[:H, :F * D] = inp["W1"][:, :F * D].to(DEV)
    d.wt = torch.full((F * D + 8, H), pad, device=DEV)
    d.wt[:F * D] = inp["W1"][:, :F * D].T.contiguous().to(DEV)
    keys = inp["keys"].long() + key_off
    sk, sp = stable_sort(keys)
    d.keys_h, d.sk_h, d.sp_h = keys, sk, sp
    d.keys, d.sk, d.sp = (t.to(torch.int32).to(DEV) for t in (keys, sk, sp))
    d.unused = inp["unused"].to(DEV)
    d.Gref, d.dwref = Gref.to(DEV), dwref.to(DEV)
    d.field_rows = (C.c_int64 * F)(*c.tables)
    for t in (d.arena, d.dhbuf, d.w, d.wt, d.ssum):
        assert t is None or t.data_ptr() % 16 == 0
    d.inputs = {n: getattr(d, n) for n in ("arena", "dhbuf", "ssum", "gfm", "w", "wt", "keys", "sk", "sp") if getattr(d, n) is not None}
    d.copies = {n: t.clone() for n, t in d.inputs.items()}
    ALL_CTX.append(d)
    return d


def extra_dx(d):
    """a gradient of x's other consumers for rp_embed_grad_gemm: dx [B + PAD_ROWS, F 64 + 4] on the device, NaN in rows >= B and
    columns >= F 64 (ldx != F D), and the statement's G with dx[b, f 64:(f + 1) 64] added to the row of pair (f, b).  Exact
    inputs: integers in -2 .. 2, two more per pair than the host file's bound counts, still far below 2^23"""
    g = torch.Generator().manual_seed(d.B + d.F)
    if d.exact:
        dx_h = torch.randint(-2, 3, (d.B, d.F * D), generator=g).float()
        assert exactness_bounds(d.inp)[0] + 2 * d.B + 1 < 2 ** 23
    else:
        dx_h = torch.randn(d.B, d.F * D, generator=g) * 1e-3 / 8
    ldx = d.F * D + 4
    dx = torch.full((d.B + PAD_ROWS, ldx), float("nan"), device=DEV)
    dx[:d.B, :d.F * D] = dx_h.to(DEV)
    ref = d.Gref.cpu().clone()
    for f in range(d.F):
        ref.index_add_(0, d.inp["base"][f] + d.inp["idx"][f], dx_h[:, f * D:(f + 1) * D].double())
    return dx, ldx, ref.to(DEV)


def looked(d, fields):
    """mask [NR] of the arena rows the pairs of `fields` look up"""
    m = torch.zeros(d.NR, dtype=torch.bool)
    for f in fields:
        m[d.inp["base"][f] + d.inp["idx"][f]] = True
    return m.to(DEV)


def new_G(d, fields):
    """the gradient arena in front of a call that covers `fields`: init in the rows somebody looks up, 7.25 in every other row
    of a table, the canary in the spare rows, NaN in the rows of the tables the call leaves out"""
    G = torch.full((d.NR, D), d.init, device=DEV)
    G[d.unused] = NEVER
    G[d.NR - SPARE_ROWS:] = CANARY_F32
    for f in range(d.F):
        if f not in fields:
            G[d.inp["base"][f]:d.inp["base"][f] + d.inp["rows"][f]] = float("nan")
    return G


def new_dw(d):
    dw = torch.full((H, d.lddw), float("nan"), device=DEV)
    dw[:, d.F * D:] = CANARY_F32
    return dw


def note(form, worst, name, share):
    worst[name] = max(worst.get(name, 0.0), share)
    per_form = WORST.setdefault(form, {})
    per_form[name] = max(per_form.get(name, 0.0), share)


def check(d, form, fields, G, G0, dw=None, dw0=None, dw_fields=None, worst=None, Gref=None):
    """G against the statement in the rows `fields` look up and bit-identical to G0 everywhere else (canary rows, rows nobody
    looks up, the tables the call leaves out); dw the same way over the columns of dw_fields (default: fields)"""
    rows = looked(d, fields)
    assert same_bits(G[~rows], G0[~rows]), f"{form}: a gradient row outside the call's pairs was written"
    Gref = d.Gref if Gref is None else Gref
    got, ref = G[rows], Gref[rows]
    if d.exact:
        assert torch.equal(got, ref.float()), f"{form}: exact-integer inputs, G differs from the float64 result"
    else:
        assert bool(torch.isfinite(got).all()), f"{form}: G is not finite"
        note(form, worst, "G", float((got.double() - ref).abs().max()) / (2e-5 * max(float((ref - d.init).abs().max()), 1e-6)))
    if dw is not None:
        cols = torch.zeros(d.lddw, dtype=torch.bool, device=DEV)
        for f in (fields if dw_fields is None else dw_fields):
            cols[f * D:(f + 1) * D] = True
        assert same_bits(dw[:, ~cols], dw0[:, ~cols]), f"{form}: dw columns outside the call's fields were written"
        got, ref = dw[:, cols], d.dwref[:, cols[:d.F * D]]
        if d.exact:
            assert torch.equal(got, ref.float()), f"{form}: exact-integer inputs, dw differs from the float64 result"
        else:
            assert bool(torch.isfinite(got).all()), f"{form}: dw is not finite"
            note(form, worst, "dw", float((got.double() - ref).abs().max()) / (2e-5 * max(float(ref.abs().max()), 1e-6)))


def report(d, form, worst):
    if not d.exact:
        print(f"\n{d.name} {form}: share of bar " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()), end="")
        assert max(worst.values()) <= 1.0, (form, worst)


# ---- the calls: every pointer and size spelled out, the workspace exactly as large as asked for --------------------------
def invoke(hip, fn, args, wsq, ws=None, short=0):
    """lib().fn(*args, workspace, bytes, stream) with a workspace of exactly wsq's bytes (0xFF inside, a guard behind) ->
    (code, workspace buffer).  short: bytes the size passed falls short of the query"""
    need = C.c_size_t(0)
    assert getattr(hip.lib(), wsq[0])(*wsq[1:], C.byref(need)) == OK, wsq
    if ws is None:
        ws = torch.full((need.value + GUARD_BYTES,), 0x5A, dtype=torch.uint8, device=DEV)
        ws[:need.value] = 0xFF
    assert ws.numel() == need.value + GUARD_BYTES and ws.data_ptr() % 256 == 0
    rc = getattr(hip.lib(), fn)(*args.values(), ws.data_ptr(), need.value - short, hip._stream())
    assert bool((ws[need.value:] == 0x5A).all()), f"{fn}: wrote behind the workspace it asked for"
    return rc, ws


def base_ptrs(d):
    off = d.key_off * D * 4
    return d.arena.data_ptr() - off


def common(d, G, acc):
    return dict(gfm=P(d.gfm), ssum=P(d.ssum), arena=base_ptrs(d), G=G.data_ptr() - d.key_off * D * 4, acc=int(d.acc if acc is None else acc))


def gemm_args(d, G, skip=0, dx=None, ldx=0, acc=None):
    return dict(sk=P(d.sk), sp=P(d.sp), n=d.F * d.B, B=d.B, D=D, dh=P(d.dhbuf), lddh=d.lddh, wt=P(d.wt), ldwt=H, dx=P(dx), ldx=ldx,
                **common(d, G, acc), skip=skip)


def reduce_args(d, G, dx, ldx, with_sum=True, acc=None, Dd=D):
    a = dict(sk=P(d.sk), sp=P(d.sp), n=d.F * d.B, B=d.B, D=Dd, dx=P(dx), ldx=ldx, **common(d, G, acc))
    if not with_sum:
        a["ssum"] = None
    return a


def seg_args(d, G, dw, skip=0, field_rows=None, acc=None):
    return dict(sk=P(d.sk), sp=P(d.sp), n=d.F * d.B, B=d.B, D=D, dh=P(d.dhbuf), lddh=d.lddh, w=P(d.w), ldw=d.ldw,
                **common(d, G, acc), skip=skip, field_rows=field_rows, dw=P(dw), lddw=d.lddw if dw is not None else 0)


def ss_args(d, G, dw, skip=0, field_rows=None, marks=None, phases=3, acc=None):
    m = (None, None, None) if marks is None else marks
    return dict(**seg_args(d, G, dw, skip, field_rows, acc), ustart=P(m[0]), ukey=P(m[1]), offs=P(m[2]), phases=phases)


def smp_tables(d, fields):
    n = len(fields)
    return ((C.c_int32 * n)(*fields), (C.c_int64 * n)(*[d.inp["base"][f] + d.key_off for f in fields]),
            (C.c_int64 * n)(*[d.inp["rows"][f] for f in fields]))


def smp_args(d, G, dw, fields, marks, phases=3, acc=None):
    fa = smp_tables(d, fields)
    return dict(keys=P(d.keys), dupq=P(marks[0]), dupkeys=P(marks[1]), B=d.B, F=d.F, fields=fa[0], base=fa[1], rows=fa[2],
                nf=len(fields), dh=P(d.dhbuf), lddh=d.lddh, w=P(d.w), ldw=d.ldw, **common(d, G, acc), dw=P(dw),
                lddw=d.lddw if dw is not None else 0, phases=phases)


def tiny_args(d, G, dw, fields, acc=None):
    n = len(fields)
    return dict(keys=P(d.keys), B=d.B, tf=(C.c_int32 * n)(*fields), tb=(C.c_int64 * n)(*[d.inp["base"][f] + d.key_off for f in fields]),
                tr=(C.c_int32 * n)(*[d.inp["rows"][f] for f in fields]), n=n, dh=P(d.dhbuf), lddh=d.lddh, wt=P(d.wt), ldwt=H,
                **common(d, G, acc), dw=P(dw), lddw=d.lddw if dw is not None else 0)


def ws_query(family, d, skip=0, nf=0, Dd=D):
    n = d.F * d.B
    return {"reduce": ("rp_embed_grad_reduce_workspace_bytes", n, Dd), "gemm": ("rp_embed_grad_reduce_workspace_bytes", n, D),
            "seg": ("rp_embed_grad_seg_workspace_bytes", n, d.B, D), "ss": ("rp_embed_grad_ss_workspace_bytes", n, d.B, D, skip),
            "smp": ("rp_embed_grad_smp_workspace_bytes", d.B, nf), "tiny": ("rp_embed_grad_tiny_workspace_bytes", d.B)}[family]


def skip_of(d, fields):
    return sum(1 << f for f in range(d.F) if f not in fields)


def guarded_i32(n, fill=-7):
    t = torch.full((n + GUARD_SLOTS,), CANARY_I32, dtype=torch.int32, device=DEV)
    t[:n] = fill
    return t


def guard_ok(t, n):
    return t.numel() == n + GUARD_SLOTS and bool((t[n:] == CANARY_I32).all())


def make_ss_marks(hip, d, fields):
    """rp_embed_grad_ss_mark into lists of exactly the documented sizes + canary slots, checked against the host's lists"""
    skip, kept = skip_of(d, fields), sorted(fields)
    nr, no = C.c_size_t(0), C.c_size_t(0)
    assert hip.lib().rp_embed_grad_ss_mark_sizes(d.B, len(kept), C.byref(nr), C.byref(no)) == OK
    assert nr.value == max(len(kept), 1) * d.B and no.value == len(kept) * ((d.B + 255) // 256) + 8
    m = (guarded_i32(nr.value), guarded_i32(nr.value), guarded_i32(no.value))
    assert hip.lib().rp_embed_grad_ss_mark(P(d.sk), d.F * d.B, d.B, skip, P(m[0]), P(m[1]), P(m[2]), hip._stream()) == OK
    assert guard_ok(m[0], nr.value) and guard_ok(m[1], nr.value) and guard_ok(m[2], no.value), "a mark list was written behind its size"
    lists, offs = ss_marks(d.sk_h, d.B, skip)
    for r_, (xs, ks) in enumerate(lists):
        assert torch.equal(m[0][r_ * d.B:r_ * d.B + xs.numel()].cpu().long(), xs), ("ustart", kept[r_])
        assert torch.equal(m[1][r_ * d.B:r_ * d.B + xs.numel()].cpu().long(), ks), ("ukey", kept[r_])
    assert torch.equal(m[2][:offs.numel()].cpu().long(), offs), "offs"
    return m


def make_smp_marks(hip, d, fields):
    nf = len(fields)
    nsc = C.c_size_t(0)
    assert hip.lib().rp_embed_grad_smp_mark_scratch(d.B, nf, C.byref(nsc)) == OK
    assert nsc.value == nf * ((d.B + 255) // 256) + 8
    m = (guarded_i32(nf * d.B), guarded_i32(nf * d.B), guarded_i32(nsc.value))
    assert hip.lib().rp_embed_grad_smp_mark(P(d.sk), P(d.sp), d.F * d.B, d.B, (C.c_int32 * nf)(*fields), nf, P(m[0]), P(m[1]), P(m[2]),
                                            hip._stream()) == OK
    assert guard_ok(m[0], nf * d.B) and guard_ok(m[1], nf * d.B) and guard_ok(m[2], nsc.value), "a mark list was written behind its size"
    dupq, dupk = smp_marks(d.sk_h, d.sp_h, d.B, fields)
    assert torch.equal(m[0][:nf * d.B].cpu().long(), dupq), "dupq"
    assert torch.equal(m[1][:nf * d.B].cpu().long(), dupk), "dupkeys: the keys of the duplicates, -1 from their count on"
    return m


def run_family(hip, d, family, fields, with_dw=True, acc=None, **how):
    """one family over `fields` of case d -> (G, G0, dw, dw0)"""
    G = new_G(d, fields)
    G0 = G.clone()
    dw = new_dw(d) if with_dw and family not in ("gemm", "reduce") else None
    dw0 = None if dw is None else dw.clone()
    skip = skip_of(d, fields)
    assert family == "smp" or d.key_off == 0, "lowered arena pointers are for rp_embed_grad_smp only (see ctx)"
    if family == "gemm":
        rc, _ = invoke(hip, "rp_embed_grad_gemm", gemm_args(d, G, skip, how.get("dx"), how.get("ldx", 0), acc), ws_query("gemm", d))
    elif family == "seg":
        rc, _ = invoke(hip, "rp_embed_grad_seg", seg_args(d, G, dw, skip, how.get("field_rows"), acc), ws_query("seg", d))
    elif family == "ss":
        q = ws_query("ss", d, skip)
        fr, marks = how.get("field_rows"), how.get("marks")
        if how.get("split"):
            rc, ws = invoke(hip, "rp_embed_grad_ss", ss_args(d, G, dw, skip, fr, marks, 1, acc), q)
            assert rc == OK
            rc, _ = invoke(hip, "rp_embed_grad_ss", ss_args(d, G, dw, skip, fr, marks, 2, acc), q, ws=ws)
        else:
            rc, _ = invoke(hip, "rp_embed_grad_ss", ss_args(d, G, dw, skip, fr, marks, 3, acc), q)
    elif family == "smp":
        q = ws_query("smp", d, nf=len(fields))
        if how.get("split"):
            rc, ws = invoke(hip, "rp_embed_grad_smp", smp_args(d, G, dw, fields, how["marks"], 1, acc), q)
            assert rc == OK
            rc, _ = invoke(hip, "rp_embed_grad_smp", smp_args(d, G, dw, fields, how["marks"], 2, acc), q, ws=ws)
        else:
            rc, _ = invoke(hip, "rp_embed_grad_smp", smp_args(d, G, dw, fields, how["marks"], 3, acc), q)
    else:
        rc, _ = invoke(hip, "rp_embed_grad_tiny", tiny_args(d, G, dw, fields, acc), ws_query("tiny", d))
    assert rc == OK, (family, rc, hip.lib().rp_last_error())
    return G, G0, dw, dw0


def agree(a, b, what):
    assert same_bits(a[0], b[0]), f"G differs between {what}"
    if a[2] is not None and b[2] is not None:
        assert same_bits(a[2], b[2]), f"dw differs between {what}"


def both(test):
    """run a test over the float inputs (the bar) and over the exact-integer inputs (torch.equal)"""
    return pytest.mark.parametrize("exact", [False, True], ids=["bar", "exact"])(test)


# ---- rp_embed_grad_gemm / rp_embed_grad_reduce ----------------------------------------------------------------------------
@both
@pytest.mark.parametrize("name", ["B1", "B127", "B128", "B129", "run-3-tiles", "long-rows", "F33-last", "T2-ragged"])
def test_gemm_and_reduce(hip, name, exact):
    # (T2-ragged: 289 tiles, so the piece list's own pass runs over several workgroups and field 2's three runs of ~4100 pairs
    #  are chained across them by the sequential walk; every smaller case leaves that walk chains of one entry)
    d = ctx(name, exact)
    every = list(range(d.F))
    worst = {}
    out = run_family(hip, d, "gemm", every)
    check(d, "gemm", every, out[0], out[1], worst=worst)
    agree(out, run_family(hip, d, "gemm", every), "two launches")
    agree(out, run_family(hip, ctx(name, exact, poison=False), "gemm", every), "poisoned and clean surroundings")
    report(d, "gemm", worst)
    # rp_embed_grad_gemm's own dx read (per pair, through the tile's sample and field tables): ldx = F 64 + 4, NaN behind
    worst = {}
    dxe, ldxe, ref = extra_dx(d)
    out = run_family(hip, d, "gemm", every, dx=dxe, ldx=ldxe)
    check(d, "gemm-dx", every, out[0], out[1], worst=worst, Gref=ref)
    agree(out, run_family(hip, d, "gemm", every, dx=dxe, ldx=ldxe), "two launches with dx")
    report(d, "gemm-dx", worst)
    # rp_embed_grad_reduce over dx = the dgrad's rows (rounded to float32: an input), ldx = F 64 + 4, NaN behind column F 64;
    # with sum_in, and in its documented mode sum_in = NULL with gfm given (only - gfm arena[key] is applied)
    ldx = d.F * D + 4
    dx = torch.full((d.B + PAD_ROWS, ldx), float("nan"), device=DEV)
    dx_h = (d.inp["dh"].double() @ d.inp["W1"].double()[:, :d.F * D]).float()
    dx[:d.B, :d.F * D] = dx_h.to(DEV)
    for with_sum in ((True, False) if d.gfm is not None else (True,)):
        worst = {}
        ref = embed_grad_reduce_f64(d.inp["arena"].masked_fill(d.inp["unused"][:, None], 0.0), d.inp["keys"], d.B, D, dx_h,
                                    d.inp["gfm"], d.inp["ssum"] if with_sum else None, d.init).to(DEV)
        outs = []
        for _ in range(2):
            G = new_G(d, every)
            G0 = G.clone()
            rc, _ = invoke(hip, "rp_embed_grad_reduce", reduce_args(d, G, dx, ldx, with_sum), ws_query("reduce", d))
            assert rc == OK
            outs.append(G)
        form = "reduce" if with_sum else "reduce-nosum"
        check(d, form, every, outs[0], G0, worst=worst, Gref=ref)
        assert same_bits(outs[0], outs[1]), "two launches"
        report(d, form, worst)


@both
@pytest.mark.parametrize("Dd", [1, 40])
def test_reduce_other_row_widths(hip, Dd, exact):
    """rp_embed_grad_reduce at D = 1 (scalar lanes) and D = 40 (float4 lanes, rows that are no power of two), B = 129, with dx
    (ldx = F D + 4), gfm and sum_in, accumulate both ways"""
    d = ctx("B129", exact)
    g = torch.Generator().manual_seed(Dd)
    rnd = (lambda shape, hi: torch.randint(-hi, hi + 1, shape, generator=g).float()) if exact else \
        (lambda shape, hi: torch.randn(shape, generator=g) * hi * 0.1)
    arena, dx_h, ssum, gfm = rnd((d.NR, Dd), 8), rnd((d.B, d.F * Dd), 2), rnd((d.B, Dd), 8), rnd((d.B,), 2)
    ldx = d.F * Dd + 4
    dx = torch.full((d.B + PAD_ROWS, ldx), float("nan"), device=DEV)
    dx[:d.B, :d.F * Dd] = dx_h.to(DEV)
    arena_d = arena.masked_fill(d.inp["unused"][:, None], float("nan")).to(DEV)
    gfm_d, ssum_d = gfm.to(DEV), ssum.to(DEV)
    rows = looked(d, range(d.F))
    for acc in (False, True):
        init = 0.5 if acc else 0.0
        ref = embed_grad_reduce_f64(arena.masked_fill(d.inp["unused"][:, None], 0.0), d.inp["keys"], d.B, Dd, dx_h, gfm, ssum, init).to(DEV)
        Gs = []
        for _ in range(2):
            G = torch.full((d.NR, Dd), init, device=DEV)
            G[d.unused] = NEVER
            G[d.NR - SPARE_ROWS:] = CANARY_F32
            G0 = G.clone()
            args = dict(sk=P(d.sk), sp=P(d.sp), n=d.F * d.B, B=d.B, D=Dd, dx=P(dx), ldx=ldx, gfm=P(gfm_d), ssum=P(ssum_d),
                        arena=P(arena_d), G=P(G), acc=int(acc))
            rc, _ = invoke(hip, "rp_embed_grad_reduce", args, ws_query("reduce", d, Dd=Dd))
            assert rc == OK
            Gs.append(G)
        assert same_bits(Gs[0], Gs[1]), "two launches"
        assert same_bits(G[~rows], G0[~rows]), "a row nobody looked up, or a canary row, was written"
        if exact:
            assert torch.equal(G[rows], ref[rows].float())
        else:
            share = float((G[rows].double() - ref[rows]).abs().max()) / (2e-5 * max(float((ref[rows] - init).abs().max()), 1e-6))
            note("reduce-D%d" % Dd, {}, "G", share)
            assert share <= 1.0, share


@both
@pytest.mark.parametrize("mask", [0x5555555555555555, 0xAAAAAAAAAAAAAAAA, 0x00000000FFFFFFFF, 0xFFFFFFFF00000000, 0x0F0F00FF3C5A9621],
                         ids=["skip-even", "skip-odd", "skip-low-half", "skip-high-half", "skip-irregular"])
def test_gemm_and_seg_64_fields_with_skip_fields(hip, mask, exact):
    """F = 64.  Every other field skipped: 32 ranges of one field each (EG_MAXG = 34), bits >= 32 both set and clear; the two
    halves (an alternating mask reads the same 32 bits wide or shifted by 32; these do not) and an irregular mask.  Every
    field has its own W1 slice and its own table: a wrong bit writes NaN-guarded rows or leaves rows at their start value.
    rp_embed_grad_gemm also with dx (ldx = F 64 + 4): its position -> (sample, field) tables under a range list"""
    d = ctx("F64", exact)
    fields = [f for f in range(64) if not (mask >> f) & 1]
    worst = {}
    out = run_family(hip, d, "gemm", fields)
    check(d, "gemm-F64", fields, out[0], out[1], worst=worst)
    agree(out, run_family(hip, d, "gemm", fields), "two launches")
    dxe, ldxe, ref = extra_dx(d)
    out = run_family(hip, d, "gemm", fields, dx=dxe, ldx=ldxe)
    check(d, "gemm-F64", fields, out[0], out[1], worst=worst, Gref=ref)
    agree(out, run_family(hip, d, "gemm", fields, dx=dxe, ldx=ldxe), "two launches with dx")
    report(d, "gemm-F64", worst)
    worst = {}
    seg = run_family(hip, d, "seg", fields)
    check(d, "seg-F64", fields, *seg, worst=worst)
    agree(seg, run_family(hip, d, "seg", fields), "two launches")
    report(d, "seg-F64", worst)


# ---- rp_embed_grad_seg ------------------------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize("name", ["small-T1", "run-3-tiles", "long-rows", "T2-ragged", "rows-asc-ties", "rows-desc", "one-run"])
def test_seg(hip, name, exact):
    d = ctx(name, exact)
    every = list(range(d.F))
    worst = {}
    out = run_family(hip, d, "seg", every, field_rows=d.field_rows)
    check(d, "seg", every, *out, worst=worst)
    agree(out, run_family(hip, d, "seg", every, field_rows=d.field_rows), "two launches")
    agree(out, run_family(hip, d, "seg", every, field_rows=None), "field_rows given and NULL (scheduling only)")
    agree(out, run_family(hip, ctx(name, exact, poison=False), "seg", every, field_rows=d.field_rows), "poisoned and clean surroundings")
    nodw = run_family(hip, d, "seg", every, with_dw=False, field_rows=d.field_rows)
    assert same_bits(out[0], nodw[0]), "G differs with and without dw"
    report(d, "seg", worst)


@both
def test_seg_33_fields_only_the_last_kept(hip, exact):
    """F = 33, skip_fields = 2^32 - 1: only field 32 is kept — a mask truncated to 32 bits keeps nothing or everything"""
    d = ctx("F33-last", exact)
    worst = {}
    for family in ("seg", "ss", "gemm"):
        out = run_family(hip, d, family, [32], field_rows=d.field_rows)
        check(d, family + "-F33", [32], *out, worst=worst)
    report(d, "seg-F33", worst)


# ---- rp_embed_grad_ss ---------------------------------------------------------------------------------------------------------
SS_CASES = ["ss-B%d" % b for b in (31, 32, 33, 255, 256, 257, 511, 513)] + ["uniq-128", "uniq-129", "long-rows", "one-run", "T2-ragged"]


@both
@pytest.mark.parametrize("name", SS_CASES)
def test_ss(hip, name, exact):
    d = ctx(name, exact)
    every = list(range(d.F))
    worst = {}
    out = run_family(hip, d, "ss", every, field_rows=d.field_rows)  # the marks made inside, phases = 3
    check(d, "ss", every, *out, worst=worst)
    agree(out, run_family(hip, d, "ss", every, field_rows=d.field_rows), "two launches")
    marks = make_ss_marks(hip, d, every)
    agree(out, run_family(hip, d, "ss", every, field_rows=d.field_rows, marks=marks), "marks made inside and ahead")
    agree(out, run_family(hip, d, "ss", every, field_rows=d.field_rows, marks=marks, split=True), "phases = 3 and 1 then 2 (marks ahead)")
    agree(out, run_family(hip, d, "ss", every, field_rows=d.field_rows, split=True), "phases = 3 and 1 then 2 (marks inside)")
    agree(out, run_family(hip, d, "ss", every, field_rows=None), "field_rows given and NULL")
    agree(out, run_family(hip, ctx(name, exact, poison=False), "ss", every, field_rows=d.field_rows), "poisoned and clean surroundings")
    if exact:
        agree(out, run_family(hip, d, "seg", every, field_rows=d.field_rows), "rp_embed_grad_ss and rp_embed_grad_seg (exact inputs)")
    report(d, "ss", worst)


# ---- rp_embed_grad_smp ----------------------------------------------------------------------------------------------------------
SMP_CASES = [("smp-B1", (0, 1), 0), ("smp-B63", (0, 1), 0), ("smp-B64", (0, 1), 0), ("smp-B65", (0, 1), 0), ("smp-distinct", (0, 1), 0),
             ("smp-pairs", (0, 1, 2), 0), ("smp-one-run", (1,), 0), ("smp-one-run", (0, 1, 2), 0), ("smp-16-fields", tuple(range(16)), 0),
             ("mix", (3, 6), 0), ("mix-acc", (1, 3, 6), 0),
             ("smp-B65", (0, 1), BIG_KEY), ("smp-pairs", (0, 1, 2), BIG_KEY)]  # keys above 2^23


@both
@pytest.mark.parametrize("name,fields,key_off", SMP_CASES,
                         ids=["%s-%dfields%s" % (n, len(f), "-keys-above-2^23" if k else "") for n, f, k in SMP_CASES])
def test_smp(hip, name, fields, exact, key_off):
    d = ctx(name, exact, key_off=key_off)
    fields = list(fields)
    worst = {}
    marks = make_smp_marks(hip, d, fields)
    out = run_family(hip, d, "smp", fields, marks=marks)
    check(d, "smp", fields, *out, worst=worst)
    agree(out, run_family(hip, d, "smp", fields, marks=marks), "two launches")
    agree(out, run_family(hip, d, "smp", fields, marks=marks, split=True), "phases = 3 and 1 then 2")
    agree(out, run_family(hip, ctx(name, exact, poison=False, key_off=key_off), "smp", fields, marks=marks), "poisoned and clean surroundings")
    nodw = run_family(hip, d, "smp", fields, with_dw=False, marks=marks)
    assert same_bits(out[0], nodw[0]), "G differs with and without dw"
    if exact and not key_off:
        agree(out, run_family(hip, d, "seg", fields, field_rows=d.field_rows), "rp_embed_grad_smp and rp_embed_grad_seg (exact inputs)")
    report(d, "smp", worst)


# ---- rp_embed_grad_tiny ---------------------------------------------------------------------------------------------------------
TINY_CASES = [("tiny-B1", (0, 2)), ("tiny-B63", (0, 2)), ("tiny-B64", (0, 2)), ("tiny-B65", (0, 2)), ("tiny-B8192", (0, 1, 3)),
              ("tiny-B8193", (0, 1, 3)), ("tiny-8", (0, 1, 2, 3, 5, 6, 7, 8)), ("tiny-9", (0, 1, 2, 3, 5, 6, 7, 8, 9)),
              ("tiny-16-224", tuple(range(16))), ("tiny-224-alone", (0,)), ("mix", (0, 2, 4)), ("one-run", (0, 1, 2))]


@both
@pytest.mark.parametrize("name,fields", TINY_CASES, ids=[n for n, _ in TINY_CASES])
@pytest.mark.parametrize("lddh", [64, 68])
def test_tiny(hip, name, fields, exact, lddh):
    """every case holds table rows nobody looks up, NaN in the arena: they must reach neither G nor dw"""
    d = ctx(name, exact, lddh=lddh)
    fields = list(fields)
    assert sum(d.inp["rows"][f] for f in fields) <= 224 and len(fields) <= 16
    worst = {}
    out = run_family(hip, d, "tiny", fields)
    check(d, "tiny", fields, *out, worst=worst)
    agree(out, run_family(hip, d, "tiny", fields), "two launches")
    agree(out, run_family(hip, ctx(name, exact, lddh=lddh, poison=False), "tiny", fields),
          "NaN and zeros in the rows nobody looks up (and the other surroundings)")
    nodw = run_family(hip, d, "tiny", fields, with_dw=False)
    assert same_bits(out[0], nodw[0]), "G differs with and without dw"
    if lddh == 68:
        agree(out, run_family(hip, ctx(name, exact), "tiny", fields), "lddh = 68 and 64")
    if exact:
        agree(out, run_family(hip, d, "seg", fields, field_rows=d.field_rows), "rp_embed_grad_tiny and rp_embed_grad_seg (exact inputs)")
    report(d, "tiny", worst)


@pytest.mark.parametrize("name,fields", [("tiny-16-224", tuple(range(16))), ("mix", (0, 2, 4)), ("tiny-B8193", (0, 1, 3))],
                         ids=["tiny-16-224", "mix", "tiny-B8193"])
def test_tiny_over_finite_tables_keeps_every_bit(hip, name, fields):
    """rp_embed_grad_tiny forms the term of a table row nobody looked up as 0 x 0 where it formed 0 x v_r before.  Over tables
    that hold finite values only (poison = False: zeros in the rows nobody looks up, as finite as any) that changes no sum,
    so G and dw keep the bits they had: on the exact-integer inputs, the float64 statement's values, element for element —
    recorded from the statement, not from a kernel.  And the same bits again with NaN in those rows."""
    d = ctx(name, True, poison=False)
    assert bool(torch.isfinite(d.arena).all()) and bool(d.unused[:d.NR - SPARE_ROWS].any())
    fields = list(fields)
    out = run_family(hip, d, "tiny", fields)
    rows, cols = looked(d, fields), torch.cat([torch.arange(f * D, (f + 1) * D) for f in fields]).to(DEV)
    assert torch.equal(out[0][rows], d.Gref[rows].float()), "G over finite tables"
    assert torch.equal(out[2][:, cols], d.dwref[:, cols].float()), "dw over finite tables"
    agree(out, run_family(hip, ctx(name, True), "tiny", fields), "finite tables and NaN in the rows nobody looks up")


@both
@pytest.mark.parametrize("family", ["gemm", "seg", "ss", "smp"])
def test_strided_dh(hip, family, exact):
    """lddh = 68 (the contract is lddh % 4 == 0), NaN in columns 64 .. 67: the same bits as with contiguous rows"""
    fields = {"gemm": [0, 1, 2], "seg": [0, 1, 2], "ss": [0, 1, 2], "smp": [0, 2]}[family]
    outs = []
    for lddh in (68, 64):
        d = ctx("smp-pairs", exact, lddh=lddh)
        how = {"marks": make_smp_marks(hip, d, fields)} if family == "smp" else {}
        outs.append(run_family(hip, d, family, fields, **how))
    worst = {}
    check(d, family + "-lddh68", fields, *outs[0], worst=worst)
    agree(outs[0], outs[1], "lddh = 68 and 64")
    report(d, family + "-lddh68", worst)


# ---- the composition ------------------------------------------------------------------------------------------------------------
@both
@pytest.mark.parametrize("name", ["mix", "mix-acc"])
def test_tiny_smp_ss_composed_as_the_autograd_node_issues_them(hip, name, exact):
    """tiny (fields 0, 2, 4), the sample-major main launch, the streaming segment-sum launch and its matrix launch (fields 1, 5;
    marks made ahead), then the launches behind the sample-major one (fields 3, 6; marks made ahead): one G, one dw that
    starts at NaN (written, not added).  Against the statement, and against rp_embed_grad_seg over every field."""
    d = ctx(name, exact)
    tiny, big, mid = [0, 2, 4], [3, 6], [1, 5]
    every = list(range(d.F))
    smp_m, ss_m = make_smp_marks(hip, d, big), make_ss_marks(hip, d, mid)
    outs = []
    for _ in range(2):
        G, dw = new_G(d, every), new_dw(d)
        G0, dw0 = G.clone(), dw.clone()
        assert invoke(hip, "rp_embed_grad_tiny", tiny_args(d, G, dw, tiny), ws_query("tiny", d))[0] == OK
        qs, qm = ws_query("smp", d, nf=len(big)), ws_query("ss", d, skip_of(d, mid))
        rc, ws_smp = invoke(hip, "rp_embed_grad_smp", smp_args(d, G, dw, big, smp_m, 1), qs)
        assert rc == OK
        rc, ws_ss = invoke(hip, "rp_embed_grad_ss", ss_args(d, G, dw, skip_of(d, mid), d.field_rows, ss_m, 1), qm)
        assert rc == OK
        assert invoke(hip, "rp_embed_grad_ss", ss_args(d, G, dw, skip_of(d, mid), d.field_rows, ss_m, 2), qm, ws=ws_ss)[0] == OK
        assert invoke(hip, "rp_embed_grad_smp", smp_args(d, G, dw, big, smp_m, 2), qs, ws=ws_smp)[0] == OK
        outs.append((G, G0, dw, dw0))
    worst = {}
    check(d, "tiny+smp+ss", every, *outs[0], worst=worst)
    agree(outs[0], outs[1], "two launches")
    seg = run_family(hip, d, "seg", every, field_rows=d.field_rows)
    check(d, "seg", every, *seg, worst=worst)
    if exact:
        agree(outs[0], seg, "the composition and rp_embed_grad_seg over every field (exact inputs)")
    else:
        rows = looked(d, every)
        scale = 2e-5 * max(float((d.Gref[rows] - d.init).abs().max()), 1e-6)
        assert float((outs[0][0][rows] - seg[0][rows]).abs().max()) <= scale
        assert float((outs[0][2][:, :d.F * D] - seg[2][:, :d.F * D]).abs().max()) <= 2e-5 * float(d.dwref.abs().max())
    report(d, "tiny+smp+ss", worst)


# ---- refusals: the documented code, no launch, no write -------------------------------------------------------------------------
def _bad(**changed):
    return lambda a, d: a.update(changed)


def _n65(a, d):
    a["n"] = 65 * d.B


REFUSALS = {
    # clause: (family, fields, what to change in the arguments, code)
    "gemm-D32": ("gemm", (0, 1, 2, 3), _bad(D=32), ERR_UNSUPPORTED),
    "seg-D32": ("seg", (0, 1, 2, 3), _bad(D=32), ERR_UNSUPPORTED),
    "ss-D32": ("ss", (0, 1, 2, 3), _bad(D=32), ERR_UNSUPPORTED),
    "gemm-lddh66": ("gemm", (0, 1, 2, 3), _bad(lddh=66), ERR_UNSUPPORTED),
    "seg-lddh66": ("seg", (0, 1, 2, 3), _bad(lddh=66), ERR_UNSUPPORTED),
    "ss-lddh66": ("ss", (0, 1, 2, 3), _bad(lddh=66), ERR_UNSUPPORTED),
    "smp-lddh66": ("smp", (1, 3), _bad(lddh=66), ERR_UNSUPPORTED),
    "tiny-lddh66": ("tiny", (0, 2), _bad(lddh=66), ERR_ARG),
    "gemm-dh-4-bytes-off": ("gemm", (0, 1, 2, 3), lambda a, d: a.update(dh=a["dh"] + 4), ERR_UNSUPPORTED),
    "seg-dh-4-bytes-off": ("seg", (0, 1, 2, 3), lambda a, d: a.update(dh=a["dh"] + 4), ERR_UNSUPPORTED),
    "ss-dh-4-bytes-off": ("ss", (0, 1, 2, 3), lambda a, d: a.update(dh=a["dh"] + 4), ERR_UNSUPPORTED),
    "smp-dh-4-bytes-off": ("smp", (1, 3), lambda a, d: a.update(dh=a["dh"] + 4), ERR_UNSUPPORTED),
    "tiny-dh-4-bytes-off": ("tiny", (0, 2), lambda a, d: a.update(dh=a["dh"] + 4), ERR_ARG),
    "gemm-F65-with-skip": ("gemm", (0, 1, 3), _n65, ERR_ARG),
    "seg-F65": ("seg", (0, 1, 2, 3), _n65, ERR_ARG),
    "ss-F65": ("ss", (0, 1, 2, 3), _n65, ERR_ARG),
    "smp-F65": ("smp", (1, 3), _bad(F=65), ERR_ARG),
    "tiny-17-tables": ("tiny", (0, 2), lambda a, d: a.update(n=17, tf=(C.c_int32 * 17)(*[0] * 17), tb=(C.c_int64 * 17)(*[0] * 17),
                                                              tr=(C.c_int32 * 17)(*[3] * 17)), ERR_ARG),
    "tiny-225-rows": ("tiny", (0, 2), lambda a, d: a.update(tr=(C.c_int32 * 2)(5, 220)), ERR_ARG),
    "tiny-255-row-table": ("tiny", (0,), lambda a, d: a.update(tr=(C.c_int32 * 1)(255)), ERR_ARG),
    "seg-gfm-without-sum": ("seg", (0, 1, 2, 3), _bad(ssum=None), ERR_ARG),
    "ss-gfm-without-sum": ("ss", (0, 1, 2, 3), _bad(ssum=None), ERR_ARG),
    "smp-gfm-without-sum": ("smp", (1, 3), _bad(ssum=None), ERR_ARG),
    "seg-lddw": ("seg", (0, 1, 2, 3), lambda a, d: a.update(lddw=d.F * D - 4), ERR_ARG),
    "ss-lddw": ("ss", (0, 1, 2, 3), lambda a, d: a.update(lddw=d.F * D - 4), ERR_ARG),
    "smp-lddw": ("smp", (1, 3), lambda a, d: a.update(lddw=d.F * D - 4), ERR_ARG),
    "tiny-lddw": ("tiny", (0, 2), _bad(lddw=3 * D - 4), ERR_ARG),  # shorter than field 2's columns
    "tiny-dw-without-arena": ("tiny", (0, 2), _bad(arena=None, gfm=None, ssum=None), ERR_ARG),
    "ss-phases-0": ("ss", (0, 1, 2, 3), _bad(phases=0), ERR_ARG),
    "ss-phases-4": ("ss", (0, 1, 2, 3), _bad(phases=4), ERR_ARG),
    "smp-phases-0": ("smp", (1, 3), _bad(phases=0), ERR_ARG),
    "smp-phases-4": ("smp", (1, 3), _bad(phases=4), ERR_ARG),
    "smp-fields-descending": ("smp", (1, 3), lambda a, d: a.update(fields=(C.c_int32 * 2)(3, 1)), ERR_ARG),
    **{f + "-workspace-one-byte-short": (f, {"smp": (1, 3), "tiny": (0, 2)}.get(f, (0, 1, 2, 3)), None, ERR_ARG)
       for f in ("reduce", "gemm", "seg", "ss", "smp", "tiny")},
}


@pytest.mark.parametrize("clause", sorted(REFUSALS))
def test_refusals_issue_no_launch_and_write_nothing(hip, clause):
    family, fields, change, code = REFUSALS[clause]
    d = ctx("refuse")
    fields = list(fields)
    G = new_G(d, fields)
    G0 = G.clone()
    dw = new_dw(d) if family not in ("gemm", "reduce") else None
    dw0 = None if dw is None else dw.clone()
    skip = skip_of(d, fields)
    if family == "reduce":
        dx = torch.zeros(d.B, d.F * D, device=DEV)
        args, fn = reduce_args(d, G, dx, d.F * D), "rp_embed_grad_reduce"
    elif family == "gemm":
        args, fn = gemm_args(d, G, skip), "rp_embed_grad_gemm"
    elif family == "seg":
        args, fn = seg_args(d, G, dw, skip, d.field_rows), "rp_embed_grad_seg"
    elif family == "ss":
        args, fn = ss_args(d, G, dw, skip, d.field_rows), "rp_embed_grad_ss"
    elif family == "smp":
        args, fn = smp_args(d, G, dw, fields, make_smp_marks(hip, d, fields)), "rp_embed_grad_smp"
    else:
        args, fn = tiny_args(d, G, dw, fields), "rp_embed_grad_tiny"
    if change is not None:
        change(args, d)
    torch.cuda.synchronize()
    n0 = hip.launch_count()
    rc, ws = invoke(hip, fn, args, ws_query(family, d, skip, len(fields)), short=1 if change is None else 0)
    torch.cuda.synchronize()
    assert rc == code, (clause, rc, hip.lib().rp_last_error())
    with pytest.raises(RuntimeError):
        hip._check(rc, clause)  # (what the wrappers do with the code)
    assert hip.launch_count() == n0, "a refused call launched"
    assert same_bits(G, G0), "a refused call wrote the gradient arena"
    assert dw is None or same_bits(dw, dw0), "a refused call wrote dw"
    assert bool((ws == 0xFF).sum() == ws.numel() - GUARD_BYTES), "a refused call wrote its workspace"
    # and the same call without the change is served
    good = run_family(hip, d, family, fields, **({"marks": make_smp_marks(hip, d, fields)} if family == "smp" else
                                                 {"field_rows": d.field_rows} if family in ("seg", "ss") else {})) \
        if family != "reduce" else None
    assert good is None or hip.launch_count() > n0


def test_mark_launches_refuse_65_fields_and_wrappers_raise(hip):
    d = ctx("refuse")
    n0 = hip.launch_count()
    m = (guarded_i32(d.F * d.B), guarded_i32(d.F * d.B), guarded_i32(d.F * 8 + 8))
    before = [t.clone() for t in m]
    assert hip.lib().rp_embed_grad_ss_mark(P(d.sk), 65 * d.B, d.B, 0, P(m[0]), P(m[1]), P(m[2]), hip._stream()) == ERR_ARG
    assert hip.lib().rp_embed_grad_smp_mark(P(d.sk), P(d.sp), 65 * d.B, d.B, (C.c_int32 * 1)(1), 1, P(m[0]), P(m[1]), P(m[2]),
                                            hip._stream()) == ERR_ARG
    assert hip.lib().rp_embed_grad_smp_mark(P(d.sk), P(d.sp), d.F * d.B, d.B, (C.c_int32 * 2)(3, 1), 2, P(m[0]), P(m[1]), P(m[2]),
                                            hip._stream()) == ERR_ARG
    need = C.c_size_t(0)
    assert hip.lib().rp_embed_grad_seg_workspace_bytes(65 * d.B, d.B, D, C.byref(need)) == ERR_ARG
    assert hip.lib().rp_embed_grad_ss_workspace_bytes(65 * d.B, d.B, D, 0, C.byref(need)) == ERR_ARG
    assert hip.lib().rp_embed_grad_smp_workspace_bytes(d.B, 17, C.byref(need)) == ERR_ARG
    # the Python wrappers: a strided dh with lddh % 4 != 0 does not fit, and the launch raises
    dh66 = torch.zeros(d.B, 66, device=DEV)[:, :64]
    assert not hip.embed_grad_seg_fits(D, 64, dh66) and not hip.embed_grad_smp_fits(D, 64, dh66)
    assert hip.embed_grad_seg_fits(D, 64, d.dhbuf[:d.B]) and not hip.embed_grad_seg_fits(32, 64, d.dhbuf[:d.B])
    G = new_G(d, range(d.F))
    G0 = G.clone()
    with pytest.raises(RuntimeError):
        hip.embed_grad_seg(d.sk, d.sp, d.B, D, dh66, d.w[:H], d.gfm[:d.B], d.ssum[:d.B], d.arena, G, False)
    torch.cuda.synchronize()
    assert hip.launch_count() == n0 and same_bits(G, G0)
    assert all(torch.equal(a, b) for a, b in zip(m, before))


def test_no_launch_wrote_an_input(hip):
    """(last in the file) the cases are uploaded once and shared: dh, ssum, gfm, W1, W1^T, the arena, the keys and the sorted
    pair list of every case used above still hold the bits they were uploaded with"""
    assert ALL_CTX
    for d in ALL_CTX:
        for n, t in d.inputs.items():
            assert torch.equal(bits(t), bits(d.copies[n])), (d.name, d.exact, n)
