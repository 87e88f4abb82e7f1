"""Every launch form of csrc/gemm.hip run alone on the device, one case of tests/test_gemm_forms.py at a time: first the
chooser must name the expected form (the launch counter, which moves once per checked launch group and not once per kernel,
must move by 1, or by the sum over the two halves of a column split: it cannot tell the short-K launches apart), then the result is held,
element by element, to bar = c_mode * sum|a||w| + u |b| against the float64 product of the same seeded fp32 inputs (the
constants and their derivation: the docstring of tests/test_gemm_forms.py).  Output buffers are prefilled with NaN inside
and a canary in their guard columns and rows: every element inside must be written, every guard element untouched bit for
bit; padding columns of the operands (and batch rows past M for the weight gradient) hold 1e3, so a tail that reads them
shows; two launches on the same inputs must be bit-identical.

ReLU needs no extra allowance under per-element bars: max(., 0) is 1-Lipschitz, so an output whose float64 pre-activation
lies within the bar of zero may land on either side (0, or a value up to the bar) and still be within the bar of the
reference — the two-sided reading test_embed_gather_linear_vs_unfused spells out with a mask.

Worst err/bar observed on the MI355X, per kernel family (printed by every test, run with -s); every err/bar <= 0.66:
  forward  f32 0.55 | short K 0.45 (bf16x6) 0.40 (bf16x3) 0.57 (bf16) | tiled 0.30 / 0.39 / 0.55 | wide 0.21 (bf16x3) 0.33 (bf16)
           column split 0.27 | row-add 0.31 / 0.36 / 0.50 | tanh, sigmoid, leaky ReLU behind each family 0.32
  wgrad    f32 0.35 | narrow 0.13 / 0.49 / 0.66 | wide 0.10 / 0.22 / 0.30 | bf16 activation 0.06 / 0.09 / 0.24
  rp_act_fwd / rp_act_bwd inside their bars, the row copies and transposes exact.  No form was found wrong.
"""
import pytest
import torch

from conftest import require_gpu
from test_gemm_forms import (ACTS, C_ACC, C_MODE, FWD_CASES, ROWADD_CASES, ROWADD_REFUSED, STEER, U, WGRAD_CASES, case_id,
                             effective_mode, fwd_bar, fwd_form, fwd_inputs, fwd_reference, precision, sample_rows, strided,
                             wgrad_form, wgrad_inputs, wgrad_reference, EXTRA_ROWS)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY = -12345.6789  # guard columns / rows of every output buffer
GUARD_ROWS = 3


@pytest.fixture(scope="module")
def hip():
    require_gpu()
    from rec_pangu_amd import hip as h
    h.lib()
    return h


def to_dev(v):
    """a strided host view on the device, with its whole buffer (padding, offset and extra rows included)"""
    if v is None:
        return None
    base = v._base if v._base is not None else v
    return base.to(DEV).as_strided(v.shape, v.stride(), v.storage_offset())


def guarded(rows, cols, ld, inside=float("nan"), dtype=torch.float32):
    """(buffer [rows + GUARD_ROWS, ld] of CANARY, its [rows, cols] view filled with `inside`)"""
    buf = torch.full((rows + GUARD_ROWS, ld), CANARY, dtype=dtype, device=DEV)
    view = buf[:rows, :cols]
    view.fill_(inside) if not isinstance(inside, torch.Tensor) else view.copy_(inside)
    return buf, view


def guards_untouched(buf, rows, cols):
    bits = buf.clone().view(torch.int32)
    canary = torch.tensor(CANARY, dtype=torch.float32).view(torch.int32).item()
    bits[:rows, :cols] = canary
    return bool((bits == canary).all())


def ratio(got, ref, bar):
    return float(((got.double().cpu() - ref).abs() / bar).max())


def launches_of(spec, form):
    family, nb = form[0], form[8]  # (the counter moves once per checked launch group: the short-K launches count as one)
    if family == "colsplit":
        mode, M, N, K, lda, ldw, a_off, w_off = spec
        return sum(launches_of(s, fwd_form(s)) for s in ((mode, M, nb, K, lda, ldw, a_off, w_off),
                                                          (mode, M, N - nb, K, lda, ldw, a_off, w_off)))
    return 1


# ---- forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,expected", FWD_CASES, ids=[case_id(s) for s, _ in FWD_CASES])
def test_linear_fwd_form(hip, spec, expected):
    mode_name, M, N, K, lda, ldw, a_off, w_off = spec
    with precision(mode_name):
        assert fwd_form(spec) == expected
        mode = effective_mode(mode_name, expected[1])
        a, w, b, aux = fwd_inputs(spec)
        rows = sample_rows(M)
        ref, absprod = fwd_reference(a, w, b, rows)
        ad, wd, bd = to_dev(a), to_dev(w), b.to(DEV)
        assert (ad.data_ptr() % 16 == 0) == (a_off % 4 == 0) and (wd.data_ptr() % 16 == 0) == (w_off % 4 == 0)
        _, auxd = strided(M, N, N + 5, 0, STEER)
        auxd.copy_(aux)
        auxd = to_dev(auxd)
        worst = {}
        for act in ACTS:
            bias = None if act == "mask" else bd  # (the mask epilogue runs with a null bias)
            pre = ref + (b.double() if bias is not None else 0.0)
            want = {"none": pre, "relu": pre.clamp_min(0), "mask": pre * (aux[rows] > 0)}[act]
            bar = fwd_bar(mode, absprod, b if bias is not None else None)
            outs = []
            for _ in range(2):
                buf, out = guarded(M, N, N + 3)
                n0 = hip.launch_count()
                hip.linear_fwd(ad, wd, bias, getattr(hip, "ACT_" + act.upper()), aux=auxd if act == "mask" else None, K=K, out=out)
                assert hip.launch_count() - n0 == launches_of(spec, expected)
                assert not bool(torch.isnan(out).any()), "an element of [M, N] was not written"
                assert guards_untouched(buf, M, N), "a guard column / row of out was written"
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), "two launches differ"
            got = outs[0][rows.to(DEV)]
            worst[act] = ratio(got, want, bar)
            if act == "relu":
                assert bool((got >= 0).all())
            if act == "mask":
                assert bool((got.cpu()[aux[rows] <= 0] == 0).all())
        print(f"\n{expected[0]} {case_id(spec)}: max err/bar " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, worst


# one case per kernel family
POST_ACT_SPECS = [("bf16x6", 389, 135, 60, 60, 64, 0, 0),          # short K: the activation is a launch of its own
                  ("bf16x6", 200, 70, 65, 68, 72, 0, 0),           # tiled
                  ("bf16x3", 65536, 256, 192, 192, 192, 0, 0),     # wide
                  ("bf16x6", 65536, 257, 65, 68, 68, 0, 0),        # column split
                  ("fp32", 129, 100, 37, 40, 40, 1, 0)]            # f32
POST_ACT_CASES = [[s for s, _ in FWD_CASES].index(spec) for spec in POST_ACT_SPECS]


@pytest.mark.parametrize("index", POST_ACT_CASES, ids=[FWD_CASES[i][1][0] + "-" + case_id(FWD_CASES[i][0]) for i in POST_ACT_CASES])
def test_linear_fwd_tanh_sigmoid_leaky_once_per_family(hip, index):
    """the activations of rp_act_apply: a launch of their own behind the short-K kernel, the epilogue of the others.  Each is
    1-Lipschitz, so the pre-activation's bar carries over; tanhf and expf of the device library are within 2 ulp, the
    sigmoid's add and divide add two more roundings: 6 u relative on top."""
    spec, expected = FWD_CASES[index]
    mode_name, M, N, K = spec[:4]
    with precision(mode_name):
        mode = effective_mode(mode_name, expected[1])
        a, w, b, _ = fwd_inputs(spec)
        rows = sample_rows(M)
        ref, absprod = fwd_reference(a, w, b, rows)
        pre = ref + b.double()
        ad, wd, bd = to_dev(a), to_dev(w), b.to(DEV)
        for name, fn in (("tanh", torch.tanh), ("sigmoid", torch.sigmoid), ("leaky", lambda t: torch.where(t > 0, t, 0.01 * t))):
            act = getattr(hip, "ACT_" + name.upper())
            buf, out = guarded(M, N, N + 3)
            n0 = hip.launch_count()
            hip.linear_fwd(ad, wd, bd, act, K=K, out=out)
            extra = 1 if expected[0] == "shortk" else 0
            assert hip.launch_count() - n0 == launches_of(spec, expected) + extra
            assert not bool(torch.isnan(out).any()) and guards_untouched(buf, M, N)
            want = fn(pre)
            r = ratio(out[rows.to(DEV)], want, fwd_bar(mode, absprod, b) + 6 * U * want.abs())
            print(f"\n{expected[0]} {name}: max err/bar {r:.3f}")
            assert r <= 1.0


# ---- weight gradient --------------------------------------------------------------------------------------------------
def _wgrad_call(hip, spec, dy, x, dw, db, accumulate):
    _, M, N, K, lddy, ldx, _, _, xb = spec
    if not xb:
        hip.linear_wgrad(dy, x, K, dw=dw, db=db, accumulate=accumulate, want_bias=False)
        return 0
    ws, nbytes = hip._workspace("linear_wgrad", M, N, K, device=dy.device)
    return hip.lib().rp_linear_wgrad_xbf16(dy.data_ptr(), lddy, x.data_ptr(), ldx, dw.data_ptr(), dw.stride(0),
                                           None if db is None else db.data_ptr(), M, N, K, int(accumulate), ws.data_ptr(),
                                           nbytes, hip._stream())


RUN_WGRAD = [(s, f) for s, f in WGRAD_CASES if f is not None]


@pytest.mark.parametrize("spec,expected", RUN_WGRAD, ids=[case_id(s) for s, _ in RUN_WGRAD])
def test_linear_wgrad_form(hip, spec, expected):
    mode_name, M, N, K, lddy, ldx, dy_off, x_off, xb = spec
    with precision(mode_name):
        assert wgrad_form(spec) == expected
        mode = effective_mode(mode_name, expected[1])
        dy, x = wgrad_inputs(spec)
        ref_w, ref_b, abs_w, abs_b = wgrad_reference(dy, x)
        dyd, xd = to_dev(dy), to_dev(x)
        assert (dyd.data_ptr() % 16 == 0) == (dy_off % 4 == 0) and xd.data_ptr() % 16 == (x_off * (2 if xb else 4)) % 16
        assert dyd._base.numel() >= dy_off + (M + EXTRA_ROWS) * lddy  # the rows past M hold 1e3 on the device too
        g = torch.Generator().manual_seed(M + N + K)
        w0, b0 = torch.randn(N, K, generator=g) * M ** 0.5, torch.randn(N, generator=g) * M ** 0.5
        worst = {}
        for accumulate, with_db in ((False, True), (True, True), (False, False)):
            outs = []
            for _ in range(2):
                wbuf, dw = guarded(N, K, K + 3, inside=w0.to(DEV) if accumulate else float("nan"))
                bbuf, db = guarded(1, N, N + 3, inside=b0.to(DEV)[None] if accumulate else float("nan"))
                n0 = hip.launch_count()
                assert _wgrad_call(hip, spec, dyd, xd, dw, db[0] if with_db else None, accumulate) == 0
                assert hip.launch_count() - n0 == 2  # the partial products, then the deterministic second-stage sum
                assert not bool(torch.isnan(dw).any()), "an element of dw was not written"
                assert guards_untouched(wbuf, N, K), "a guard column / row of dw was written"
                if with_db:
                    assert not bool(torch.isnan(db).any()) and guards_untouched(bbuf, 1, N)
                else:
                    assert bool(torch.isnan(db).all()) and guards_untouched(bbuf, 1, N), "db = NULL, yet db was written"
                outs.append((dw, db))
            assert torch.equal(outs[0][0], outs[1][0]), "two launches differ"
            want_w = ref_w + (w0.double() if accumulate else 0.0)
            want_b = ref_b + (b0.double() if accumulate else 0.0)
            tag = ("acc" if accumulate else "set") + ("" if with_db else "-nodb")
            # (accumulating rounds once more: u of the sum)
            worst["dw " + tag] = ratio(outs[0][0], want_w, C_MODE[mode] * abs_w + (U * want_w.abs() if accumulate else 0.0))
            if with_db:
                assert torch.equal(outs[0][1], outs[1][1])
                worst["db " + tag] = ratio(outs[0][1][0], want_b, C_ACC * abs_b + (U * want_b.abs() if accumulate else 0.0))
        print(f"\nwgrad-{expected[0]} {case_id(spec)}: max err/bar " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert max(worst.values()) <= 1.0, worst


REFUSED_WGRAD = [s for s, f in WGRAD_CASES if f is None]


@pytest.mark.parametrize("spec", REFUSED_WGRAD, ids=[case_id(s) for s in REFUSED_WGRAD])
def test_linear_wgrad_xbf16_refuses(hip, spec):
    mode_name, M, N, K = spec[:4]
    with precision(mode_name):
        assert wgrad_form(spec) is None
        dy, x = wgrad_inputs(spec)
        wbuf, dw = guarded(N, K, K + 3)
        n0 = hip.launch_count()
        rc = _wgrad_call(hip, spec, to_dev(dy), to_dev(x), dw, None, False)
        torch.cuda.synchronize()
        assert rc == -3 and b"N < 128" in hip.lib().rp_last_error()
        assert hip.launch_count() == n0 and bool(torch.isnan(dw).all()) and guards_untouched(wbuf, N, K)


# ---- rp_linear_fwd_rowadd ---------------------------------------------------------------------------------------------
def _rowadd_call(hip, a, w, out, M, N, K, rs, radd, add_cols):
    return hip.lib().rp_linear_fwd_rowadd(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0),
                                          M, N, K, rs.data_ptr(), radd.data_ptr(), radd.stride(0), add_cols, hip._stream())


def _rowadd_inputs(M, N, K, lda, ldw, a_off, w_off):
    a, w, _, _ = fwd_inputs(("", M, N, K, lda, ldw, a_off, w_off))
    g = torch.Generator().manual_seed(M + N + K)
    rs = torch.randn(M, generator=g)
    _, radd = strided(M, 64, 72, 0, STEER)
    radd.copy_(torch.randn(M, 64, generator=g))
    return a, w, rs, radd


@pytest.mark.parametrize("case", ROWADD_CASES, ids=[case_id(c) for c in ROWADD_CASES])
def test_linear_fwd_rowadd(hip, case):
    """out = a w^T + rs[m] radd[m, n % 64] for n < add_cols, against float64; the added term is one fp32 multiply-add on
    top of the product: 2 u of its own magnitude and of the result"""
    mode, M, N, K, add_cols = case
    with precision(mode):
        a, w, rs, radd = _rowadd_inputs(M, N, K, (K + 7) // 4 * 4, (K + 3) // 4 * 4, 0, 0)
        rows = torch.arange(M)
        ref, absprod = fwd_reference(a, w, None, rows)
        add = (rs.double()[:, None] * radd.double()).repeat(1, N // 64)
        add[:, add_cols:] = 0
        want = ref + add
        bar = C_MODE[mode] * absprod + 2 * U * (add.abs() + want.abs())
        ad, wd, rsd, raddd = to_dev(a), to_dev(w), rs.to(DEV), to_dev(radd)
        outs = []
        for _ in range(2):
            buf, out = guarded(M, N, N + 3)
            n0 = hip.launch_count()
            assert _rowadd_call(hip, ad, wd, out, M, N, K, rsd, raddd, add_cols) == 0
            assert hip.launch_count() - n0 == 1
            assert not bool(torch.isnan(out).any()) and guards_untouched(buf, M, N)
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        r = ratio(outs[0], want, bar)
        print(f"\nrowadd {case_id(case)}: max err/bar {r:.3f}")
        assert r <= 1.0
        if add_cols == 0:  # nothing added: the plain short-K product, bit for bit
            assert torch.equal(outs[0], hip.linear_fwd(ad, wd, None, hip.ACT_NONE, K=K))


@pytest.mark.parametrize("clause", sorted(ROWADD_REFUSED))
def test_linear_fwd_rowadd_refuses(hip, clause):
    mode, M, N, K, lda, ldw, a_off, w_off, add_cols = ROWADD_REFUSED[clause]
    with precision(mode):
        a, w, rs, radd = _rowadd_inputs(M, N, K, lda, ldw, a_off, w_off)
        buf, out = guarded(M, N, N + 3)
        n0 = hip.launch_count()
        rc = _rowadd_call(hip, to_dev(a), to_dev(w), out, M, N, K, rs.to(DEV), to_dev(radd), add_cols)
        torch.cuda.synchronize()
        assert rc == -3, clause
        assert hip.launch_count() == n0 and bool(torch.isnan(out).all()) and guards_untouched(buf, M, N)
    with precision("bf16x6"):  # and the same call with the clause mended is served
        a, w, rs, radd = _rowadd_inputs(128, 64, 64, 64, 64, 0, 0)
        buf, out = guarded(128, 64, 67)
        assert _rowadd_call(hip, to_dev(a), to_dev(w), out, 128, 64, 64, rs.to(DEV), to_dev(radd), 64) == 0


# ---- the small launches -----------------------------------------------------------------------------------------------
SIZES = (1, 5, 37, 64, 1677)
SMALL = [(R, Cc) for R in SIZES for Cc in SIZES] + [(5000, 300)]  # the last: more rows than one grid covers, the kernels loop


@pytest.mark.parametrize("R,Cc", SMALL)
def test_row_copies_and_transposes_are_exact(hip, R, Cc):
    g = torch.Generator().manual_seed(R * 7 + Cc)
    _, src = strided(R, Cc, Cc + 3, 1, STEER)
    src.copy_(torch.randn(R, Cc, generator=g))
    srcd = to_dev(src)
    lib, st = hip.lib(), hip._stream()
    dst0 = torch.randn(R, Cc, generator=g)
    # rp_copy_rows / rp_add_rows into a buffer with another unaligned stride and guards
    buf, out = guarded(R, Cc, Cc + 5)
    assert lib.rp_copy_rows(srcd.data_ptr(), srcd.stride(0), out.data_ptr(), out.stride(0), R, Cc, st) == 0
    assert torch.equal(out.cpu(), src) and guards_untouched(buf, R, Cc)
    buf, out = guarded(R, Cc, Cc + 5, inside=dst0.to(DEV))
    assert lib.rp_add_rows(srcd.data_ptr(), srcd.stride(0), out.data_ptr(), out.stride(0), R, Cc, st) == 0
    assert torch.equal(out.cpu(), dst0 + src) and guards_untouched(buf, R, Cc)
    # rp_transpose: out [C_out, R], rows C .. C_out - 1 zero; rp_transpose_copy: the same and an untransposed copy
    c_out = Cc + 2
    buf, out = guarded(c_out, R, R + 3)
    assert lib.rp_transpose(srcd.data_ptr(), srcd.stride(0), out.data_ptr(), out.stride(0), R, Cc, c_out, st) == 0
    want = torch.cat([src.t(), torch.zeros(2, R)])
    assert torch.equal(out.cpu(), want) and guards_untouched(buf, c_out, R)
    buf, out = guarded(c_out, R, R + 3)
    cbuf, copy = guarded(R, Cc, Cc + 6)
    assert lib.rp_transpose_copy(srcd.data_ptr(), srcd.stride(0), out.data_ptr(), out.stride(0), R, Cc, c_out, copy.data_ptr(),
                                 copy.stride(0), st) == 0
    assert torch.equal(out.cpu(), want) and guards_untouched(buf, c_out, R)
    assert torch.equal(copy.cpu(), src) and guards_untouched(cbuf, R, Cc)


@pytest.mark.parametrize("R,Cc", SMALL)
def test_act_fwd_and_bwd_vs_float64(hip, R, Cc):
    """rp_act_fwd / rp_act_bwd at unaligned leading dimensions.  Forward: tanhf / expf within 2 ulp, the sigmoid two more
    roundings: 6 u relative (ReLU and leaky ReLU: one rounding at most).  Backward: dy * f(y) from the stored fp32 output y,
    three roundings of terms no larger than |dy|: 4 u |dy|."""
    g = torch.Generator().manual_seed(R * 11 + Cc)
    _, x = strided(R, Cc, Cc + 3, 1, STEER)
    x.copy_(torch.randn(R, Cc, generator=g) * 3)
    _, dy = strided(R, Cc, Cc + 1, 2, STEER)
    dy.copy_(torch.randn(R, Cc, generator=g))
    xd, dyd = to_dev(x), to_dev(dy)
    lib, st = hip.lib(), hip._stream()
    xx = x.double()
    fwd = {"relu": xx.clamp_min(0), "tanh": torch.tanh(xx), "sigmoid": torch.sigmoid(xx), "leaky": torch.where(xx > 0, xx, 0.01 * xx)}
    for name, want in fwd.items():
        act = getattr(hip, "ACT_" + name.upper())
        ybuf, y = guarded(R, Cc, Cc + 5)
        assert lib.rp_act_fwd(xd.data_ptr(), xd.stride(0), y.data_ptr(), y.stride(0), R, Cc, act, st) == 0
        assert guards_untouched(ybuf, R, Cc)
        r = ratio(y, want, 6 * U * want.abs() + 1e-45)
        yy = y.cpu().double()  # the backward reads the fp32 output it is given
        grad = {"relu": (yy > 0).double(), "tanh": 1 - yy * yy, "sigmoid": yy * (1 - yy),
                "leaky": torch.where(yy > 0, 1.0, 0.01).double()}[name]
        obuf, out = guarded(R, Cc, Cc + 7)
        assert lib.rp_act_bwd(dyd.data_ptr(), dyd.stride(0), y.data_ptr(), y.stride(0), out.data_ptr(), out.stride(0), R, Cc, act,
                              st) == 0
        assert not bool(torch.isnan(out).any()) and guards_untouched(obuf, R, Cc)
        rb = ratio(out, dy.double() * grad, 4 * U * dy.double().abs() + 1e-45)
        assert r <= 1.0 and rb <= 1.0, (name, r, rb)
        if name == "relu":
            rbuf, rout = guarded(R, Cc, Cc + 7)
            assert lib.rp_relu_bwd(dyd.data_ptr(), dyd.stride(0), y.data_ptr(), y.stride(0), rout.data_ptr(), rout.stride(0), R,
                                   Cc, st) == 0
            assert torch.equal(rout, out) and torch.equal(out.cpu(), dy * (y.cpu() > 0)) and guards_untouched(rbuf, R, Cc)
