"""Which launch form of csrc/gemm.hip serves a shape (rp_linear_fwd_form / rp_linear_wgrad_form: host functions, no GPU),
and the error bars the one-form-at-a-time GPU tests (tests/test_hip_gemm_forms.py, which imports CASES, the input draws,
the float64 references and the bars from here) hold every form to.

FWD_CASES / WGRAD_CASES: (precision, shape, strides, pointer offsets) -> the expected form tuple.  The tuples are literals:
they are the specification, recorded from the dispatch as it stood when the choice was gathered into one function.
REACHABLE is every instantiation the dispatch macros of gemm.hip can emit, written out; the cases together must select
exactly that set, so a form added later without a case fails here.

The bars.  bar[m, n] = c_mode * sum_k |a[m,k]| |w[n,k]| + u * |b[n]|  (wgrad: the sum runs over the batch), u = 2^-24.
  accumulation, every mode: the kernels accumulate in fp32 over the contraction length L.  The worst case is L u, useless
    at L = 65536.  The test inputs are drawn with zero mean, and for zero-mean data the rounding errors of a length-L fp32
    sum are, with probability 1 - 2 exp(-lambda^2 / 2), below lambda * u * sqrt(sum_k s_k^2), s_k the partial sums (Higham
    & Mary, "Sharper probabilistic backward error analysis for random data", SIAM J. Sci. Comput. 42 (2020)); the partial
    sums of zero-mean terms grow like sqrt(k), which makes that bound about 1.1 * lambda * u * sum|a||w| for every L.
    lambda = 7 leaves 2 exp(-24.5) = 5e-11 per element, against some 1e9 elements compared by the whole file:
    C_ACC = 8 u.
  fp32:   C_ACC.
  bf16x6: each operand is cut (by truncation, exactly) into three 8-bit pieces p0 + p1 + p2, |p1| < 2^-7 |x|,
    |p2| < 2^-15 |x|; six of the nine products are taken, the dropped p1.p2 + p2.p1 + p2.p2 are below
    (2 * 2^-22 + 2^-30) |a||w| < 2^-21 |a||w|:  C_ACC + 2^-21.
  bf16x3: hi = RN_bf16(x), lo = RN_bf16(x - hi), 2^-9 relative per rounding (the header's figure for a bf16 rounding), so
    the low piece's rounding leaves 2^-18 |x| per operand and the dropped lo.lo product 2^-18 |a||w|:  C_ACC + 3 * 2^-18.
  bf16:   2^-9 per operand, (1 + 2^-9)^2 - 1:  C_ACC + 2^-8 + 2^-18.
  db (the bias gradient) is an fp32 column sum in every mode: C_ACC * sum_m |dy[m, n]|.
Condition 1 (test_cpu_emulation_sits_inside_the_bars): an emulation of each mode — the operands split with torch.bfloat16
arithmetic as the kernels split them, the piece products exact in float64, accumulated one after the other in fp32, the
worst order there is — stays inside the bar for every case, on the host.  Condition 2
(test_bars_are_no_looser_than_the_existing_tolerances): at the shapes shared with test_linear_fwd / test_linear_wgrad of
tests/test_hip_kernels.py, every element's bar is below that test's atol + rtol |ref|.  (test_linear_wgrad's 65536 x 64 x 64
is not among the shared shapes: its atol there, 2e-6 sqrt(M) * 40, is 8.2 u of sum|dy||x|, about the accumulation term alone;
the six-product constant above is the worst case of the dropped products and cannot go below 16 u.  The many-splits case
of this file has 40000 rows, and that test keeps its shape and its tolerance.)"""
import ctypes

import pytest
import torch

from rec_pangu_amd import hip

U = 2.0 ** -24
C_ACC = 8 * U
C_MODE = {"fp32": C_ACC, "bf16x6": C_ACC + 2.0 ** -21, "bf16x3": C_ACC + 3 * 2.0 ** -18, "bf16": C_ACC + 2.0 ** -8 + 2.0 ** -18}
NPROD_MODE = {0: "fp32", 6: "bf16x6", 3: "bf16x3", 1: "bf16"}
STEER = 1e3  # what the padding columns / rows hold: a tail that reads them lands far above any bar
SAMPLE = 256  # rows compared of a large-M forward case: the first and last SAMPLE and SAMPLE in between

# ((precision, M, N, K, lda, ldw, a_off, w_off), (family, nprod, tile, VEC_A, VEC_W, short-K launches, per, grid, split Nb))
# a_off / w_off: floats between a 16-byte boundary and the operand's first element
FWD_CASES = [
    # ---- tiled: every tile shape x VEC_A x VEC_W x product count.  128x64x4w is the `else` shape: M <= 64 with K > 64
    (('bf16x6', 24, 16, 100, 100, 104, 0, 0), ('tiled', 6, '128x64x4w', True, True, (), 0, (1, 1), 0)),
    (('bf16x6', 24, 16, 100, 100, 104, 0, 1), ('tiled', 6, '128x64x4w', True, False, (), 0, (1, 1), 0)),
    (('bf16x6', 24, 16, 100, 101, 104, 0, 0), ('tiled', 6, '128x64x4w', False, True, (), 0, (1, 1), 0)),
    (('bf16x6', 24, 16, 100, 100, 101, 1, 0), ('tiled', 6, '128x64x4w', False, False, (), 0, (1, 1), 0)),
    (('bf16x6', 200, 70, 65, 68, 72, 0, 0), ('tiled', 6, '128x64x8w', True, True, (), 0, (2, 2), 0)),
    (('bf16x6', 200, 70, 65, 68, 72, 0, 1), ('tiled', 6, '128x64x8w', True, False, (), 0, (2, 2), 0)),
    (('bf16x6', 200, 70, 65, 69, 72, 0, 0), ('tiled', 6, '128x64x8w', False, True, (), 0, (2, 2), 0)),
    (('bf16x6', 200, 70, 65, 68, 65, 1, 0), ('tiled', 6, '128x64x8w', False, False, (), 0, (2, 2), 0)),
    (('bf16x6', 65536, 256, 65, 68, 72, 0, 0), ('tiled', 6, '128x128', True, True, (), 0, (512, 2), 0)),
    (('bf16x6', 65536, 256, 65, 68, 72, 0, 1), ('tiled', 6, '128x128', True, False, (), 0, (512, 2), 0)),
    (('bf16x6', 65536, 256, 65, 69, 72, 0, 0), ('tiled', 6, '128x128', False, True, (), 0, (512, 2), 0)),
    (('bf16x6', 65536, 256, 65, 68, 65, 1, 0), ('tiled', 6, '128x128', False, False, (), 0, (512, 2), 0)),
    (('bf16x3', 24, 16, 100, 100, 104, 0, 0), ('tiled', 3, '128x64x4w', True, True, (), 0, (1, 1), 0)),
    (('bf16x3', 24, 16, 100, 100, 104, 0, 1), ('tiled', 3, '128x64x4w', True, False, (), 0, (1, 1), 0)),
    (('bf16x3', 24, 16, 100, 101, 104, 0, 0), ('tiled', 3, '128x64x4w', False, True, (), 0, (1, 1), 0)),
    (('bf16x3', 24, 16, 100, 100, 101, 1, 0), ('tiled', 3, '128x64x4w', False, False, (), 0, (1, 1), 0)),
    (('bf16x3', 200, 70, 65, 68, 72, 0, 0), ('tiled', 3, '128x64x8w', True, True, (), 0, (2, 2), 0)),
    (('bf16x3', 200, 70, 65, 68, 72, 0, 1), ('tiled', 3, '128x64x8w', True, False, (), 0, (2, 2), 0)),
    (('bf16x3', 200, 70, 65, 69, 72, 0, 0), ('tiled', 3, '128x64x8w', False, True, (), 0, (2, 2), 0)),
    (('bf16x3', 200, 70, 65, 68, 65, 1, 0), ('tiled', 3, '128x64x8w', False, False, (), 0, (2, 2), 0)),
    (('bf16x3', 65536, 256, 65, 68, 72, 0, 0), ('tiled', 3, '128x128', True, True, (), 0, (512, 2), 0)),
    (('bf16x3', 65536, 256, 65, 68, 72, 0, 1), ('tiled', 3, '128x128', True, False, (), 0, (512, 2), 0)),
    (('bf16x3', 65536, 256, 65, 69, 72, 0, 0), ('tiled', 3, '128x128', False, True, (), 0, (512, 2), 0)),
    (('bf16x3', 65536, 256, 65, 68, 65, 1, 0), ('tiled', 3, '128x128', False, False, (), 0, (512, 2), 0)),
    (('bf16', 24, 16, 100, 100, 104, 0, 0), ('tiled', 1, '128x64x4w', True, True, (), 0, (1, 1), 0)),
    (('bf16', 24, 16, 100, 100, 104, 0, 1), ('tiled', 1, '128x64x4w', True, False, (), 0, (1, 1), 0)),
    (('bf16', 24, 16, 100, 101, 104, 0, 0), ('tiled', 1, '128x64x4w', False, True, (), 0, (1, 1), 0)),
    (('bf16', 24, 16, 100, 100, 101, 1, 0), ('tiled', 1, '128x64x4w', False, False, (), 0, (1, 1), 0)),
    (('bf16', 200, 70, 65, 68, 72, 0, 0), ('tiled', 1, '128x64x8w', True, True, (), 0, (2, 2), 0)),
    (('bf16', 200, 70, 65, 68, 72, 0, 1), ('tiled', 1, '128x64x8w', True, False, (), 0, (2, 2), 0)),
    (('bf16', 200, 70, 65, 69, 72, 0, 0), ('tiled', 1, '128x64x8w', False, True, (), 0, (2, 2), 0)),
    (('bf16', 200, 70, 65, 68, 65, 1, 0), ('tiled', 1, '128x64x8w', False, False, (), 0, (2, 2), 0)),
    (('bf16', 65536, 256, 65, 68, 72, 0, 0), ('tiled', 1, '128x128', True, True, (), 0, (512, 2), 0)),
    (('bf16', 65536, 256, 65, 68, 72, 0, 1), ('tiled', 1, '128x128', True, False, (), 0, (512, 2), 0)),
    (('bf16', 65536, 256, 65, 69, 72, 0, 0), ('tiled', 1, '128x128', False, True, (), 0, (512, 2), 0)),
    (('bf16', 65536, 256, 65, 68, 65, 1, 0), ('tiled', 1, '128x128', False, False, (), 0, (512, 2), 0)),
    (('bf16x6', 131072, 64, 65, 68, 68, 0, 0), ('tiled', 6, '128x64x4w', True, True, (), 0, (1024, 1), 0)),  # 1024 tiles, not big
    # ---- short K: interior + right + bottom in every product count
    (('bf16x6', 389, 135, 60, 60, 64, 0, 0), ('shortk', 6, None, True, True, ('interior', 'right', 'bottom'), 1, (3, 2), 0)),
    (('bf16x3', 389, 135, 60, 60, 64, 0, 0), ('shortk', 3, None, True, True, ('interior', 'right', 'bottom'), 1, (3, 2), 0)),
    (('bf16', 389, 135, 60, 60, 64, 0, 0), ('shortk', 1, None, True, True, ('interior', 'right', 'bottom'), 1, (3, 2), 0)),
    (('bf16x6', 129, 100, 37, 37, 37, 0, 0), ('shortk', 6, None, False, False, ('guarded',), 1, (2, 2), 0)),  # nothing aligned
    (('bf16x6', 256, 128, 4, 8, 4, 0, 0), ('shortk', 6, None, True, True, ('interior',), 1, (2, 2), 0)),  # select-to-zero columns
    (('bf16x6', 256, 128, 8, 8, 12, 0, 0), ('shortk', 6, None, True, True, ('interior',), 1, (2, 2), 0)),
    (('bf16x3', 256, 64, 60, 64, 60, 0, 0), ('shortk', 3, None, True, True, ('interior',), 1, (2, 1), 0)),
    # per = 2 column tiles per workgroup, three interior tiles: the second workgroup's tile1 is clamped
    (('bf16x6', 49285, 199, 64, 64, 64, 0, 0), ('shortk', 6, None, True, True, ('interior', 'right', 'bottom'), 2, (385, 2), 0)),
    (('bf16x6', 777, 64, 64, 64, 64, 0, 0), ('shortk', 6, None, True, True, ('interior', 'bottom'), 1, (6, 1), 0)),
    (('bf16x6', 513, 1, 64, 64, 64, 0, 0), ('shortk', 6, None, True, True, ('guarded',), 1, (5, 1), 0)),  # the 64 -> 1 head
    (('bf16', 128, 64, 64, 64, 64, 0, 1), ('shortk', 1, None, True, False, ('guarded',), 1, (1, 1), 0)),  # misaligned w pointer
    (('auto', 300, 1677, 64, 64, 64, 0, 0), ('shortk', 6, None, True, True, ('interior', 'right', 'bottom'), 1, (2, 26), 0)),
    # ---- the 256 x 128 wide kernel
    (('bf16x3', 65536, 256, 192, 192, 192, 0, 0), ('wide', 3, None, True, True, (), 0, (512, 1), 0)),
    (('bf16', 65536, 256, 192, 196, 192, 0, 0), ('wide', 1, None, True, True, (), 0, (512, 1), 0)),
    # ---- the two-launch column split: [M, 256] + one column, and [M, 256] (wide kernel) + four columns
    (('bf16x6', 65536, 257, 65, 68, 68, 0, 0), ('colsplit', 6, None, True, True, (), 0, (0, 0), 256)),
    (('bf16x3', 65536, 260, 192, 192, 192, 0, 0), ('colsplit', 3, None, True, True, (), 0, (0, 0), 256)),
    # ---- the f32 kernel
    (('fp32', 200, 70, 65, 68, 68, 0, 0), ('f32', 0, None, True, True, (), 0, (2, 2), 0)),
    (('fp32', 200, 70, 65, 68, 67, 0, 0), ('f32', 0, None, True, False, (), 0, (2, 2), 0)),
    (('fp32', 200, 70, 65, 65, 68, 0, 0), ('f32', 0, None, False, True, (), 0, (2, 2), 0)),
    (('fp32', 200, 70, 65, 65, 67, 0, 0), ('f32', 0, None, False, False, (), 0, (2, 2), 0)),
    (('fp32', 129, 100, 37, 40, 40, 1, 0), ('f32', 0, None, False, True, (), 0, (2, 2), 0)),
]

# ((precision, M, N, K, lddy, ldx, dy_off, x_off, x is bf16), (family, nprod, NA, VEC_X, VEC_Y, S, rows, grid) or None = refused)
# dy_off in floats, x_off in elements of x (bf16 elements for a bf16 activation)
WGRAD_CASES = [
    (('bf16x6', 24, 16, 43, 16, 64, 0, 0, 0), ('narrow', 6, 1, True, False, 1, 32, (1, 1, 1))),
    (('bf16x6', 513, 100, 37, 100, 37, 0, 0, 0), ('narrow', 6, 1, False, False, 17, 32, (1, 2, 17))),
    (('bf16x6', 300, 520, 40, 520, 40, 0, 0, 0), ('wide', 6, 2, True, False, 10, 32, (80, 1, 1))),   # ragged N (the MMOE 520)
    (('bf16x6', 129, 200, 37, 201, 37, 1, 0, 0), ('wide', 6, 2, False, False, 5, 32, (16, 1, 1))),   # odd ldx; S = 5 of 8
    (('bf16x6', 200, 100, 37, 100, 38, 0, 2, 1), ('xbf16', 6, 1, True, False, 7, 32, (1, 2, 7))),
    (('bf16x3', 24, 16, 43, 16, 64, 0, 0, 0), ('narrow', 3, 1, True, False, 1, 32, (1, 1, 1))),
    (('bf16x3', 513, 100, 37, 100, 37, 0, 0, 0), ('narrow', 3, 1, False, False, 17, 32, (1, 2, 17))),
    (('bf16x3', 300, 520, 40, 520, 40, 0, 0, 0), ('wide', 3, 2, True, False, 10, 32, (80, 1, 1))),
    (('bf16x3', 129, 200, 37, 201, 37, 1, 0, 0), ('wide', 3, 2, False, False, 5, 32, (16, 1, 1))),
    (('bf16x3', 200, 100, 37, 100, 38, 0, 2, 1), ('xbf16', 3, 1, True, False, 7, 32, (1, 2, 7))),
    (('bf16', 24, 16, 43, 16, 64, 0, 0, 0), ('narrow', 1, 1, True, False, 1, 32, (1, 1, 1))),
    (('bf16', 513, 100, 37, 100, 37, 0, 0, 0), ('narrow', 1, 1, False, False, 17, 32, (1, 2, 17))),
    (('bf16', 300, 520, 40, 520, 40, 0, 0, 0), ('wide', 1, 2, True, False, 10, 32, (80, 1, 1))),
    (('bf16', 129, 200, 37, 201, 37, 1, 0, 0), ('wide', 1, 2, False, False, 5, 32, (16, 1, 1))),
    (('bf16', 200, 100, 37, 100, 38, 0, 2, 1), ('xbf16', 1, 1, True, False, 7, 32, (1, 2, 7))),
    (('bf16x6', 333, 1, 64, 1, 64, 0, 0, 1), ('xbf16', 6, 1, True, False, 11, 32, (1, 1, 11))),
    (('bf16x6', 333, 64, 33, 64, 34, 0, 2, 1), ('xbf16', 6, 1, True, False, 11, 32, (1, 1, 11))),
    (('bf16x6', 333, 127, 40, 128, 48, 0, 6, 1), ('xbf16', 6, 1, True, False, 11, 32, (1, 2, 11))),
    (('bf16x6', 300, 128, 40, 128, 42, 0, 2, 0), ('wide', 6, 2, True, False, 10, 32, (16, 1, 1))),   # x 8-byte aligned only
    (('bf16x6', 20000, 130, 130, 132, 132, 0, 0, 0), ('wide', 6, 2, True, False, 125, 160, (512, 1, 1))),
    (('bf16x6', 40000, 64, 64, 64, 64, 0, 0, 0), ('narrow', 6, 1, True, False, 417, 96, (1, 1, 417))),  # one tile, many splits
    (('auto', 2048, 512, 649, 512, 672, 0, 0, 0), ('wide', 3, 2, True, False, 22, 96, (576, 1, 1))),
    (('fp32', 513, 100, 37, 100, 40, 0, 0, 0), ('f32', 0, 0, True, True, 17, 32, (1, 2, 17))),
    (('fp32', 513, 100, 37, 100, 37, 0, 0, 0), ('f32', 0, 0, False, True, 17, 32, (1, 2, 17))),
    (('fp32', 513, 100, 37, 101, 40, 0, 0, 0), ('f32', 0, 0, True, False, 17, 32, (1, 2, 17))),
    (('fp32', 513, 100, 37, 101, 37, 0, 0, 0), ('f32', 0, 0, False, False, 17, 32, (1, 2, 17))),
    (('fp32', 24, 16, 43, 16, 64, 1, 2, 0), ('f32', 0, 0, False, False, 1, 32, (1, 1, 1))),
    # what rp_linear_wgrad_xbf16 refuses, one clause each: N = 128, odd ldx, x 2 bytes off, the fp32 mode
    (('bf16x6', 200, 128, 37, 128, 38, 0, 0, 1), None),
    (('bf16x6', 200, 100, 37, 100, 39, 0, 0, 1), None),
    (('bf16x6', 200, 100, 37, 100, 38, 0, 1, 1), None),
    (('fp32', 200, 100, 37, 100, 38, 0, 0, 1), None),
]

# rp_linear_fwd_rowadd has no chooser (one kernel, one grid rule): (precision, M, N, K, add_cols), the whole cross product
# in the six-product mode, one shape in the others
ROWADD_CASES = ([("bf16x6", M, N, K, add) for M in (128, 384) for N in (64, 192) for K in (4, 60, 64)
                 for add in sorted({0, 64, N})] + [("bf16x3", 384, 192, 60, 64), ("bf16", 384, 192, 60, 192)])
# every clause of its refusal, one case each: (precision, M, N, K, lda, ldw, a_off, w_off, add_cols).  Three of the cases
# cannot isolate their clause: any K in 1..3 also breaks K % 4, any M in 1..127 also M % 128, any N in 1..63 also N % 64
# (and a zero dimension makes an empty operand, whose null pointer is refused earlier, as a bad argument).
ROWADD_REFUSED = {
    "fp32 mode": ("fp32", 128, 64, 64, 64, 64, 0, 0, 64), "K < 4": ("bf16x6", 128, 64, 3, 4, 4, 0, 0, 64),
    "K > 64": ("bf16x6", 128, 64, 68, 68, 68, 0, 0, 64), "K % 4": ("bf16x6", 128, 64, 62, 64, 64, 0, 0, 64),
    "M < 128": ("bf16x6", 64, 64, 64, 64, 64, 0, 0, 64), "M % 128": ("bf16x6", 200, 64, 64, 64, 64, 0, 0, 64),
    "N < 64": ("bf16x6", 128, 32, 64, 64, 64, 0, 0, 0), "N % 64": ("bf16x6", 128, 100, 64, 64, 64, 0, 0, 64),
    "add_cols < 0": ("bf16x6", 128, 64, 64, 64, 64, 0, 0, -64), "add_cols % 64": ("bf16x6", 128, 64, 64, 64, 64, 0, 0, 32),
    "add_cols > N": ("bf16x6", 128, 64, 64, 64, 64, 0, 0, 128), "lda % 4": ("bf16x6", 128, 64, 64, 65, 64, 0, 0, 64),
    "ldw % 4": ("bf16x6", 128, 64, 64, 64, 66, 0, 0, 64), "a misaligned": ("bf16x6", 128, 64, 64, 64, 64, 1, 0, 64),
    "w misaligned": ("bf16x6", 128, 64, 64, 64, 64, 0, 2, 64),
}

ACTS = ("none", "relu", "mask")
# every instantiation the dispatch of gemm.hip can emit, one entry each
REACHABLE = {
    # linear_fwd_kernel<VEC_A, VEC_W>
    ("fwd_f32", True, True), ("fwd_f32", True, False), ("fwd_f32", False, True), ("fwd_f32", False, False),
    # linear_fwd_bf16_smallk_kernel<NPROD, ACT, FULL>
    ("fwd_shortk", 6, "none", True), ("fwd_shortk", 6, "relu", True), ("fwd_shortk", 6, "mask", True),
    ("fwd_shortk", 6, "none", False), ("fwd_shortk", 6, "relu", False), ("fwd_shortk", 6, "mask", False),
    ("fwd_shortk", 3, "none", True), ("fwd_shortk", 3, "relu", True), ("fwd_shortk", 3, "mask", True),
    ("fwd_shortk", 3, "none", False), ("fwd_shortk", 3, "relu", False), ("fwd_shortk", 3, "mask", False),
    ("fwd_shortk", 1, "none", True), ("fwd_shortk", 1, "relu", True), ("fwd_shortk", 1, "mask", True),
    ("fwd_shortk", 1, "none", False), ("fwd_shortk", 1, "relu", False), ("fwd_shortk", 1, "mask", False),
    # linear_fwd_bf16_smallk_kernel<NPROD, RP_ACT_NONE, true, ROWADD = true>
    ("fwd_rowadd", 6), ("fwd_rowadd", 3), ("fwd_rowadd", 1),
    # linear_fwd_bf16_wide_kernel<NPROD>
    ("fwd_wide", 3), ("fwd_wide", 1),
    # linear_fwd_bf16_kernel<NPROD, tile, VEC_A, VEC_W>
    ("fwd_tiled", 6, "128x128", True, True), ("fwd_tiled", 6, "128x128", True, False),
    ("fwd_tiled", 6, "128x128", False, True), ("fwd_tiled", 6, "128x128", False, False),
    ("fwd_tiled", 6, "128x64x8w", True, True), ("fwd_tiled", 6, "128x64x8w", True, False),
    ("fwd_tiled", 6, "128x64x8w", False, True), ("fwd_tiled", 6, "128x64x8w", False, False),
    ("fwd_tiled", 6, "128x64x4w", True, True), ("fwd_tiled", 6, "128x64x4w", True, False),
    ("fwd_tiled", 6, "128x64x4w", False, True), ("fwd_tiled", 6, "128x64x4w", False, False),
    ("fwd_tiled", 3, "128x128", True, True), ("fwd_tiled", 3, "128x128", True, False),
    ("fwd_tiled", 3, "128x128", False, True), ("fwd_tiled", 3, "128x128", False, False),
    ("fwd_tiled", 3, "128x64x8w", True, True), ("fwd_tiled", 3, "128x64x8w", True, False),
    ("fwd_tiled", 3, "128x64x8w", False, True), ("fwd_tiled", 3, "128x64x8w", False, False),
    ("fwd_tiled", 3, "128x64x4w", True, True), ("fwd_tiled", 3, "128x64x4w", True, False),
    ("fwd_tiled", 3, "128x64x4w", False, True), ("fwd_tiled", 3, "128x64x4w", False, False),
    ("fwd_tiled", 1, "128x128", True, True), ("fwd_tiled", 1, "128x128", True, False),
    ("fwd_tiled", 1, "128x128", False, True), ("fwd_tiled", 1, "128x128", False, False),
    ("fwd_tiled", 1, "128x64x8w", True, True), ("fwd_tiled", 1, "128x64x8w", True, False),
    ("fwd_tiled", 1, "128x64x8w", False, True), ("fwd_tiled", 1, "128x64x8w", False, False),
    ("fwd_tiled", 1, "128x64x4w", True, True), ("fwd_tiled", 1, "128x64x4w", True, False),
    ("fwd_tiled", 1, "128x64x4w", False, True), ("fwd_tiled", 1, "128x64x4w", False, False),
    # linear_wgrad_partial_kernel<VEC_Y, VEC_X>
    ("wgrad_f32", True, True), ("wgrad_f32", True, False), ("wgrad_f32", False, True), ("wgrad_f32", False, False),
    # linear_wgrad_bf16_kernel<NPROD, NA, PF, VEC_X>
    ("wgrad_bf16", 6, 1, True), ("wgrad_bf16", 6, 1, False), ("wgrad_bf16", 6, 2, True), ("wgrad_bf16", 6, 2, False),
    ("wgrad_bf16", 3, 1, True), ("wgrad_bf16", 3, 1, False), ("wgrad_bf16", 3, 2, True), ("wgrad_bf16", 3, 2, False),
    ("wgrad_bf16", 1, 1, True), ("wgrad_bf16", 1, 1, False), ("wgrad_bf16", 1, 2, True), ("wgrad_bf16", 1, 2, False),
    # linear_wgrad_bf16_kernel<NPROD, 1, 1, true, X_BF16 = true>
    ("wgrad_xbf16", 6), ("wgrad_xbf16", 3), ("wgrad_xbf16", 1),
}


def case_id(spec):
    return "-".join(str(v) for v in spec)


class precision:
    """the matmul precision of the library for a block, then `auto` again (the library's default)"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        hip.set_matmul_precision(self.mode)

    def __exit__(self, *exc):
        hip.set_matmul_precision("auto")


def fwd_form(spec, act=hip.ACT_NONE):
    """the chooser's answer for a forward case, as the tuple FWD_CASES holds (call under precision(spec[0]))"""
    _, M, N, K, lda, ldw, a_off, w_off = spec
    f = hip.linear_fwd_form(M, N, K, lda, ldw, a_off % 4 == 0, w_off % 4 == 0, act)
    return (f["family"], f["nprod"], f["tile"], f["vec_a"], f["vec_w"], f["sk"], f["per"], f["grid"], f["split_nb"])


def x_align(x_off, x_bf16):
    nbytes = x_off * (2 if x_bf16 else 4)
    return next(a for a in (16, 8, 4, 2, 1) if nbytes % a == 0)


def wgrad_form(spec):
    _, M, N, K, lddy, ldx, dy_off, x_off, xb = spec
    f = hip.linear_wgrad_form(M, N, K, lddy, ldx, dy_off % 4 == 0, x_align(x_off, xb), bool(xb))
    return None if f is None else (f["family"], f["nprod"], f["na"], f["vec_x"], f["vec_y"], f["S"], f["rows"], f["grid"])


def fwd_instantiations(spec, form):
    """the kernel instantiations a forward case runs over the epilogues ACTS (a column split: those of its two launches)"""
    family, nprod, tile, va, vw, sk, _, _, nb = form
    if family == "f32":
        return {("fwd_f32", va, vw)}
    if family == "tiled":
        return {("fwd_tiled", nprod, tile, va, vw)}
    if family == "wide":
        return {("fwd_wide", nprod)}
    if family == "shortk":
        full = {"interior": True, "right": False, "bottom": False, "guarded": False}
        return {("fwd_shortk", nprod, act, full[launch]) for act in ACTS for launch in sk}
    mode, M, N, K, lda, ldw, a_off, w_off = spec
    out = set()
    for n in (nb, N - nb):  # (w + nb * ldw keeps the alignment of w: nb is a multiple of 128)
        sub = (mode, M, n, K, lda, ldw, a_off, w_off)
        out |= fwd_instantiations(sub, fwd_form(sub))
    return out


def wgrad_instantiation(form):
    family, nprod, na, vx, vy = form[:5]
    return {"f32": ("wgrad_f32", vy, vx), "xbf16": ("wgrad_xbf16", nprod)}.get(family, ("wgrad_bf16", nprod, na, vx))


# ---- the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec,expected", FWD_CASES, ids=[case_id(s) for s, _ in FWD_CASES])
def test_forward_form(spec, expected):
    with precision(spec[0]):
        assert fwd_form(spec) == expected
        for act in (hip.ACT_RELU, hip.ACT_MASK):  # the fused epilogues change nothing of the form
            assert fwd_form(spec, act) == expected
        for act in (hip.ACT_TANH, hip.ACT_SIGMOID, hip.ACT_LEAKY):  # the others follow the short-K kernel as a launch
            f = hip.linear_fwd_form(*spec[1:6], spec[6] % 4 == 0, spec[7] % 4 == 0, act)
            assert f["post_act"] == (expected[0] == "shortk")


@pytest.mark.parametrize("spec,expected", WGRAD_CASES, ids=[case_id(s) for s, _ in WGRAD_CASES])
def test_wgrad_form(spec, expected):
    with precision(spec[0]):
        assert wgrad_form(spec) == expected
        if expected is None:
            assert b"N < 128" in hip.lib().rp_last_error()  # (the message said N <= 128; N = 128 is refused)
        if spec[8] and expected is not None:  # the fp32 activation at the same place has a form of its own
            assert hip.linear_wgrad_form(*spec[1:6], True, 16, False)["family"] in ("narrow", "wide")


def test_cases_cover_every_reachable_instantiation():
    seen = set()
    for spec, expected in FWD_CASES:
        with precision(spec[0]):
            seen |= fwd_instantiations(spec, fwd_form(spec))
    for spec, expected in WGRAD_CASES:
        if expected is not None:
            seen.add(wgrad_instantiation(expected))
    seen |= {("fwd_rowadd", {"bf16x6": 6, "bf16x3": 3, "bf16": 1}[c[0]]) for c in ROWADD_CASES}
    assert seen == REACHABLE, (sorted(REACHABLE - seen, key=str), sorted(seen - REACHABLE, key=str))


def test_form_functions_validate_and_read_the_precision_in_force():
    lib = hip.lib()
    o = (ctypes.c_int * 16)()
    assert lib.rp_linear_fwd_form(8, 8, 8, 8, 8, 1, 1, 0, None) == -1 and b"null" in lib.rp_last_error()
    assert lib.rp_linear_fwd_form(8, 8, 8, 7, 8, 1, 1, 0, o) == -1
    assert lib.rp_linear_fwd_form(8, 8, 8, 8, 8, 1, 1, 9, o) == -1
    assert lib.rp_linear_wgrad_form(8, 8, 8, 8, 7, 1, 16, 0, o) == -1
    assert lib.rp_linear_wgrad_form(0, 8, 8, 8, 8, 1, 16, 0, o) == -1
    got = []
    for mode in ("fp32", "bf16", "bf16x3", "bf16x6", "auto"):
        with precision(mode):
            got.append((hip.linear_fwd_form(4096, 64, 64, 64, 64)["nprod"], hip.linear_wgrad_form(4096, 64, 64, 64, 64)["nprod"],
                        hip.linear_fwd_form(65536, 1024, 1677, 1680, 1680)["nprod"]))
    assert got == [(0, 0, 0), (1, 1, 1), (3, 3, 3), (6, 6, 6), (6, 6, 3)]  # auto: three products when matrix-core bound


# ---- threshold neighbours: the shape on each side of every threshold of the dispatch ----------------------------------
def _fwd(mode, M, N, K, ld=None, a16=True, w16=True):
    ld = ld or (K + 3) // 4 * 4
    with precision(mode):
        f = hip.linear_fwd_form(M, N, K, ld, ld, a16, w16)
    return f["family"], f["tile"]


def test_threshold_neighbours():
    # K = 64 / 65: short K ends
    assert _fwd("bf16x6", 24, 16, 64) == ("shortk", None) and _fwd("bf16x6", 24, 16, 65) == ("tiled", "128x64x4w")
    # M = 64 / 65 (K > 64, a small grid): four waves up to 64 rows, eight from there
    assert _fwd("bf16x6", 64, 16, 100) == ("tiled", "128x64x4w") and _fwd("bf16x6", 65, 16, 100) == ("tiled", "128x64x8w")
    # 1024 tiles of 128 x 64: eight waves below, four from there
    assert _fwd("bf16x6", 131072 - 128, 64, 65) == ("tiled", "128x64x8w") and _fwd("bf16x6", 131072 - 127, 64, 65) == ("tiled", "128x64x4w")
    # 1024 tiles of 128 x 128 and N = 255 / 256: the 128 x 128 tile
    assert _fwd("bf16x6", 65536, 256, 65) == ("tiled", "128x128") and _fwd("bf16x6", 65536 - 128, 256, 65) == ("tiled", "128x64x4w")
    assert _fwd("bf16x6", 65536 - 128, 256, 65, 68)[1] == "128x64x4w" and _fwd("bf16x6", 32768 - 128, 256, 65)[1] == "128x64x8w"
    assert _fwd("bf16x6", 131072, 255, 65) == ("tiled", "128x64x4w") and _fwd("bf16x6", 131072, 256, 65) == ("tiled", "128x128")
    # pad <= N / 8: 341 columns pad to 384 by 43 > 341 / 8 = 42.6, 342 by 42 <= 42.75 (M large enough that the split,
    # which needs 1024 tiles of the whole 128-column part, and the 128 x 128 tile, which counts the padded part, differ)
    assert _fwd("bf16x6", 49152, 342, 65) == ("tiled", "128x128") and _fwd("bf16x6", 49152, 341, 65) == ("tiled", "128x64x4w")
    # the column split: N = 256 has nothing left over, 257 has; 1024 tiles of its whole part
    assert _fwd("bf16x6", 65536, 257, 65) == ("colsplit", None) and _fwd("bf16x6", 65536 - 128, 257, 65)[0] == "tiled"
    assert _fwd("bf16x3", 65536, 255, 192)[0] == "tiled"
    # the wide kernel: 512 tiles, M % 256, K = 191 / 192, N = 255 / 256 (N % 32), two-piece modes, aligned operands
    assert _fwd("bf16x3", 65536, 256, 192) == ("wide", None) and _fwd("bf16", 65536, 256, 192) == ("wide", None)
    assert _fwd("bf16x3", 65536 - 256, 256, 192)[0] == "tiled" and _fwd("bf16x3", 65536 + 128, 256, 192)[0] == "tiled"
    assert _fwd("bf16x3", 65536, 256, 191, 192)[0] == "tiled" and _fwd("bf16x6", 65536, 256, 192)[0] == "tiled"
    assert _fwd("bf16x3", 65536, 288, 192)[0] == "colsplit" and _fwd("bf16x3", 32768, 288, 192) == ("tiled", "128x64x4w")
    assert _fwd("bf16x3", 65536, 256, 192, a16=False)[0] == "tiled" and _fwd("bf16x3", 65536, 256, 192, 193)[0] == "tiled"
    # wgrad: N = 127 / 128 narrow / wide; the fp32 mode has no wide form
    with precision("bf16x6"):
        assert hip.linear_wgrad_form(300, 127, 40, 128, 40)["family"] == "narrow"
        assert hip.linear_wgrad_form(300, 128, 40, 128, 40)["family"] == "wide"
        assert hip.linear_wgrad_form(300, 127, 40, 128, 40, True, 4, True)["family"] == "xbf16"
        assert hip.linear_wgrad_form(300, 128, 40, 128, 40, True, 4, True) is None
        assert hip.linear_wgrad_form(300, 64, 40, 64, 40, True, 4)["vec_x"] is False  # 8-byte rows need an 8-byte pointer
        assert hip.linear_wgrad_form(300, 64, 40, 64, 40, True, 8)["vec_x"] is True
    with precision("fp32"):
        assert hip.linear_wgrad_form(300, 128, 40, 128, 40)["family"] == "f32"
        assert hip.linear_wgrad_form(300, 64, 40, 64, 40, True, 8)["vec_x"] is False  # (16-byte rows in the f32 kernel)


# ---- the batch-split plan ---------------------------------------------------------------------------------------------
TN_BM = 32


@pytest.mark.parametrize("mode", ["fp32", "bf16x6", "auto"])
def test_wgrad_plan_properties(mode):
    lib = hip.lib()
    n = ctypes.c_size_t(0)
    with precision(mode):
        for M in (1, 31, 32, 33, 513, 4099, 20000, 65536, 65537, 1 << 20):
            for N in (1, 16, 64, 100, 127, 128, 130, 512, 520, 1024):
                for K in (1, 37, 64, 128, 129, 649, 1677):
                    f = hip.linear_wgrad_form(M, N, K, N, K)
                    S, rows = f["S"], f["rows"]
                    assert (S - 1) * rows < M <= S * rows, (M, N, K, S, rows)
                    assert rows % TN_BM == 0 and rows >= TN_BM and 1 <= S <= 512, (M, N, K, S, rows)
                    assert lib.rp_linear_wgrad_workspace_bytes(M, N, K, ctypes.byref(n)) == 0
                    assert n.value == (S * N * K + S * N) * 4 + 256, (M, N, K)  # what the entry point asks of its caller
                    wide = f["family"] == "wide"
                    assert wide == (mode != "fp32" and N >= 128)
                    kt, nt = -(-K // 128), -(-N // (128 if wide else 64))
                    # the wide 1-D grid holds whole groups of eight splits: the blocks of splits S .. 8 ceil(S / 8) - 1 return
                    assert f["grid"] == ((8 * -(-S // 8) * kt * nt, 1, 1) if wide else (kt, nt, S))


# ---- inputs, float64 references, bars: shared with the GPU tests ----------------------------------------------------------
def strided(rows, cols, ld, off, fill, extra_rows=0):
    """a [rows, cols] view with row stride ld whose first element lies `off` elements into a fresh buffer filled with
    `fill`: (buffer, view).  extra_rows more rows of the buffer follow the view."""
    buf = torch.full((off + (rows + extra_rows) * ld,), fill, dtype=torch.float32)
    return buf, buf[off:off + rows * ld].view(rows, ld)[:, :cols]


def fwd_inputs(spec, want_aux=True):
    """seeded fp32 operands of a forward case, the padding columns of a and w holding STEER: a, w (strided views), b, aux.
    The draws are zero-mean, and C_ACC holds for zero-mean operands only: a case with biased inputs needs a bar of its own."""
    _, M, N, K, lda, ldw, a_off, w_off = spec
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    _, a = strided(M, K, lda, a_off, STEER)
    _, w = strided(N, K, ldw, w_off, STEER)
    a.copy_(torch.randn(M, K, generator=g))
    w.copy_(torch.randn(N, K, generator=g) / K ** 0.5)
    b = torch.randn(N, generator=g)
    aux = torch.randn(M, N, generator=g) if want_aux else None  # asymmetric: a transposed read of it shows
    return a, w, b, aux


def sample_rows(M):
    if M <= 4 * SAMPLE:
        return torch.arange(M)
    g = torch.Generator().manual_seed(M)
    mid = torch.randint(SAMPLE, M - SAMPLE, (SAMPLE,), generator=g)
    return torch.cat([torch.arange(SAMPLE), mid, torch.arange(M - SAMPLE, M)])


def fwd_reference(a, w, b, rows):
    """float64 pre-activation without bias and sum_k |a||w| of the sampled rows"""
    ad, wd = a[rows].double(), w.double()
    return ad @ wd.t(), ad.abs() @ wd.abs().t()


def fwd_bar(mode, absprod, b):
    return C_MODE[mode] * absprod + (U * b.double().abs() if b is not None else 0.0)


def effective_mode(mode, nprod):
    return NPROD_MODE[nprod] if mode == "auto" else mode


def wgrad_inputs(spec):
    """dy [M, N], x [M, K] (fp32, or bf16 when the case says so); the padding columns and EXTRA rows past M hold STEER.
    Zero-mean draws, as C_ACC assumes (see fwd_inputs)."""
    _, M, N, K, lddy, ldx, dy_off, x_off, xb = spec
    g = torch.Generator().manual_seed(1000 * M + 10 * N + K + 1)
    _, dy = strided(M, N, lddy, dy_off, STEER, extra_rows=EXTRA_ROWS)
    _, x = strided(M, K, ldx, x_off, STEER, extra_rows=EXTRA_ROWS)
    dy.copy_(torch.randn(M, N, generator=g))
    x.copy_(torch.randn(M, K, generator=g))
    if xb:
        buf = torch.full((x_off + (M + EXTRA_ROWS) * ldx,), STEER, dtype=torch.bfloat16)
        x16 = buf[x_off:x_off + M * ldx].view(M, ldx)[:, :K]
        x16.copy_(x)  # (round to nearest even)
        x = x16
    return dy, x


EXTRA_ROWS = 40  # more than one 32-row stage past M


def wgrad_reference(dy, x):
    """float64 dw, db and the sums of absolute products (a bf16 activation widens exactly)"""
    yd, xd = dy.double(), x.double()
    return yd.t() @ xd, yd.sum(dim=0), yd.abs().t() @ xd.abs(), yd.abs().sum(dim=0)


# ---- Condition 1: an emulation of each mode stays inside the bar -------------------------------------------------------
def bf16_pieces(x, mode):
    """the bf16 pieces (as float64) a kernel cuts an fp32 operand into, and the piece pairs whose products it takes"""
    if mode == "fp32":
        return [x.double()], [(0, 0)]
    if mode == "bf16x6":  # three pieces by truncation: the top 16 bits of what is left, three times (exact)
        pieces, rest = [], x.clone()
        for _ in range(3):
            p = (rest.view(torch.int32) & -65536).view(torch.float32)
            pieces.append(p.double())
            rest = rest - p
        assert bool((rest == 0).all())
        return pieces, [(0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)]  # smallest terms first
    hi = x.to(torch.bfloat16).float()
    if mode == "bf16":
        return [hi.double()], [(0, 0)]
    lo = (x - hi).to(torch.bfloat16).float()
    return [hi.double(), lo.double()], [(0, 1), (1, 0), (0, 0)]


def emulate(a, w, mode):
    """sum_k a[m,k] w[n,k] the way `mode` computes it, accumulated in fp32 one product after the other (serial order: the
    worst there is; the kernels sum in blocks).  a: [M, L], w: [N, L] fp32 (a bf16 operand: widened first)."""
    pa, pairs = bf16_pieces(a.float().contiguous(), mode)
    pw, _ = bf16_pieces(w.float().contiguous(), mode)
    # [L, M, N] products per piece pair, exact in float64 (a product of two bf16 pieces is exact in fp32 too)
    prods = [pa[i].t()[:, :, None] * pw[j].t()[:, None, :] for i, j in pairs]
    acc = torch.zeros(a.shape[0], w.shape[0], dtype=torch.float32)
    if mode == "fp32":  # one fused multiply-add per term: the exact product enters the fp32 sum
        for p in prods[0]:
            acc = (acc.double() + p).float()
        return acc
    prods = [p.float() for p in prods]
    for k in range(a.shape[1]):
        for p in prods:
            acc += p[k]
    return acc


def _ratio(got, ref, bar):
    return float(((got.double() - ref).abs() / bar).max())


def test_cpu_emulation_sits_inside_the_bars():
    worst = {}
    for spec, form in FWD_CASES:
        mode = effective_mode(spec[0], form[1])
        a, w, b, _ = fwd_inputs(spec, want_aux=False)
        rows = sample_rows(spec[1])[::37] if spec[1] > 1024 else sample_rows(spec[1])[::7]
        ref, absprod = fwd_reference(a, w, b, rows)
        got = (emulate(a[rows], w, mode).double() + b.double()).float()
        r = _ratio(got, ref + b.double(), fwd_bar(mode, absprod, b))
        worst[mode] = max(worst.get(mode, 0.0), r)
        assert r <= 1.0, (spec, r)
    for spec, form in WGRAD_CASES:
        if form is None:
            continue
        mode = effective_mode(spec[0], form[1])
        dy, x = wgrad_inputs(spec)
        if spec[1] > 1024:  # (a corner of the output: the serial loop runs over the batch)
            dy, x = dy[:, :6], x[:, :5]
        ref_w, ref_b, abs_w, abs_b = wgrad_reference(dy, x)
        r = _ratio(emulate(dy.t(), x.t(), mode), ref_w, C_MODE[mode] * abs_w)
        rb = _ratio(emulate(dy.t(), torch.ones(1, dy.shape[0]), "fp32")[:, 0], ref_b, C_ACC * abs_b)
        worst[mode] = max(worst.get(mode, 0.0), r)
        worst["db"] = max(worst.get("db", 0.0), rb)
        assert r <= 1.0 and rb <= 1.0, (spec, r, rb)
    print("worst emulated err/bar:", {k: round(v, 3) for k, v in sorted(worst.items())})


# ---- Condition 2: no looser than the tolerances of the existing tests at the shapes they share --------------------------
FWD_TOL = {"fp32": (1e-5, 2e-5), "bf16x6": (1e-5, 2e-5), "bf16x3": (1e-4, 2e-4), "bf16": (5e-2, 5e-2)}  # test_linear_fwd
WGRAD_SLACK = {"fp32": 1.0, "bf16x6": 1.0, "bf16x3": 20.0, "bf16": 3000.0}  # test_linear_wgrad


def test_bars_are_no_looser_than_the_existing_tolerances():
    shared_fwd = {(777, 64, 64), (513, 1, 64), (300, 1677, 64), (129, 100, 37)}  # shapes of test_linear_fwd among FWD_CASES
    shared_wgrad = {(24, 16, 43), (513, 100, 37), (2048, 512, 649)}  # and of test_linear_wgrad
    n = 0
    for spec, form in FWD_CASES:
        if spec[1:4] in shared_fwd:
            mode = effective_mode(spec[0], form[1])
            a, w, b, _ = fwd_inputs(spec, want_aux=False)
            ref, absprod = fwd_reference(a, w, b, torch.arange(spec[1]))
            rtol, atol = FWD_TOL[mode]
            assert bool((fwd_bar(mode, absprod, b) <= atol + rtol * (ref + b.double()).abs()).all()), spec
            n += 1
    for spec, form in WGRAD_CASES:
        if spec[1:4] in shared_wgrad and form is not None and not spec[8]:
            mode = effective_mode(spec[0], form[1])
            dy, x = wgrad_inputs(spec)
            ref_w, ref_b, abs_w, abs_b = wgrad_reference(dy, x)
            slack = WGRAD_SLACK[mode]
            tol = 2e-6 * spec[1] ** 0.5 * 4 * slack
            assert bool((C_MODE[mode] * abs_w <= tol * 10 + 1e-4 * slack * ref_w.abs()).all()), spec
            assert bool((C_ACC * abs_b <= tol * 10 + 1e-4 * ref_b.abs()).all()), spec
            n += 1
    assert n >= 12, n
