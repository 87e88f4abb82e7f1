"""CPU-side checks of the drop-in boundary: the shared object loads, exports every symbol that
include/rec_pangu_hip.h declares (and nothing undeclared), the ctypes table covers them all, argument
validation works without a GPU, and no product module reaches into oracle/."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT


def _declared():
    text = open(os.path.join(ROOT, "include", "rec_pangu_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rp_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_exactly_the_header():
    from rec_pangu_amd import hip
    assert os.path.exists(hip.LIB_PATH), "build with __graft_entry__.build() / make -C rec_pangu_amd/csrc"
    declared = _declared()
    assert declared, "no declarations parsed"
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(set(re.findall(r" T (rp_[a-z0-9_]+)", out)))
    assert exported == declared
    assert sorted(hip.EXPORTED_SYMBOLS) == declared, "ctypes signature table out of sync with the header"
    lib = hip.lib()
    for name in declared:
        assert getattr(lib, name) is not None


def test_argument_validation_needs_no_gpu():
    from rec_pangu_amd import hip
    lib = hip.lib()
    from rec_pangu_amd import hip as _hip
    assert lib.rp_version() == _hip.ABI_VERSION  # (the bindings refuse a library of another version)
    n = ctypes.c_size_t(0)
    assert lib.rp_linear_wgrad_workspace_bytes(65536, 64, 1677, ctypes.byref(n)) == 0 and n.value > 0
    assert lib.rp_loss_partials(65536) >= 1
    # null pointers / bad sizes are refused with an error code and a message, never a crash
    rc = lib.rp_linear_fwd(None, 0, None, 0, None, None, 0, 1, 1, 1, 0, None, 0, None)
    assert rc == -1 and b"null" in lib.rp_last_error()
    rc = lib.rp_embed_gather_fwd(None, None, None, None, 0, None, 0, 1, 1, None, 0, None, None, None, None, None)
    assert rc == -1
    rc = lib.rp_adam_step(None, None, None, None, None, 0, 0.0, 0.0, 0.0, 0.0, 1, 0, None, None, None)
    assert rc == -1


def test_missing_library_fails_loudly(monkeypatch):
    from rec_pangu_amd import hip
    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", "/nonexistent/librecpangu_hip.so")
    with pytest.raises(RuntimeError, match="no fallback"):
        hip.lib()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "rec_pangu_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports oracle/"
                assert "ref_ops" not in src, f"{f} references the oracle"


def test_cin_pair_gather_lists_cover_every_pair_once_per_member():
    """Host logic of rp_cin_pair_bwd_x (rec_pangu_amd.hip.cin_pair_lists): for every field h the lists of all pair-tile
    halves together name each pair containing h exactly once per membership — the diagonal pair (h,h) twice — with
    the right partner and the right local row; and the forward's pair order is the row-major upper triangle."""
    import torch
    from rec_pangu_amd import hip
    for H in (1, 2, 5, 26, 32):
        lstart, lent = hip.cin_pair_lists(H, torch.device("cpu"))
        lstart, lent = lstart.tolist(), lent.tolist()
        pairs = [(h, m) for h in range(H) for m in range(h, H)]
        ntile = (len(pairs) + 127) // 128
        assert len(lstart) == 2 * ntile * H + 1
        seen = {h: [] for h in range(H)}
        for tile in range(ntile):
            for half in range(2):
                lo = tile * 128 + half * 64
                for h in range(H):
                    li = (2 * tile + half) * H + h
                    for e in lent[lstart[li]:lstart[li + 1]]:
                        pl, m = e & 255, e >> 8
                        assert 0 <= pl < 64 and lo + pl < len(pairs)
                        assert sorted(pairs[lo + pl]) == sorted((h, m)), (H, tile, half, h, pl, m)
                        seen[h].append(lo + pl)
        for h in range(H):
            want = sorted([p for p, (a, b) in enumerate(pairs) if a == h or b == h] +
                          [p for p, (a, b) in enumerate(pairs) if a == h and b == h])
            assert sorted(seen[h]) == want, (H, h)
    # symmetric pair weights: row-major upper triangle, off-diagonal entries summed
    W = torch.arange(2 * 3 * 3, dtype=torch.float32).view(2, 3, 3)
    from oracle.ref_pieces import cin_pair_ws
    ws = cin_pair_ws(W)
    ref = torch.stack([torch.stack([W[o, 0, 0], W[o, 0, 1] + W[o, 1, 0], W[o, 0, 2] + W[o, 2, 0], W[o, 1, 1],
                                    W[o, 1, 2] + W[o, 2, 1], W[o, 2, 2]]) for o in range(2)])
    assert torch.equal(ws, ref)


# ---- the ctypes table and the RP_* constants are parsed from the header ----------------------------------------------
_vp, _i64, _i32, _sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
_f32, _f64, _u64 = ctypes.c_float, ctypes.c_double, ctypes.c_uint64
# literal rows of the hand-written table the parser replaced; together they hold every kind of type of the header.  Typed
# host out-parameters (size_t *, int *, the char buffer of rp_plan_launch_name) are c_void_p like every pointer.
EXPECTED_SIGNATURES = {
    "rp_embed_grad_ss": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _u64, _vp,
                                        _vp, _i64, _vp, _vp, _vp, _i32, _vp, _sz, _vp]),  # uint64_t mid-list, 25 arguments
    "rp_lazy_adam_flush_deferred": (ctypes.c_int, [_i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _f64, _f64, _f64, _vp, _i64,
                                                   _vp, _vp]),
    "rp_field_attention_fwd": (ctypes.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _i64, _vp]),
    "rp_fill_words": (ctypes.c_int, [_vp, _i64, ctypes.c_uint32, _vp]),
    "rp_binary_metrics": (ctypes.c_int, [_vp, _sz, _vp, _vp, _i64, _f64, _i32, _vp, _vp]),  # a struct pointer among them
    "rp_pieces_ld": (ctypes.c_int64, [_i32, _i32]),
    "rp_last_error": (ctypes.c_char_p, []),
    "rp_launch_count": (ctypes.c_uint64, []),
    "rp_plan_launch_name": (ctypes.c_int, [_vp, _i32, _vp, _i32, _vp]),
    "rp_sort_workspace_bytes": (ctypes.c_int, [_i64, _vp]),
}


@pytest.mark.parametrize("name", sorted(EXPECTED_SIGNATURES))
def test_parsed_signature_is_the_hand_written_one(name):
    from rec_pangu_amd import hip
    res, args = hip._SIGNATURES[name]
    assert (res, list(args)) == EXPECTED_SIGNATURES[name]
    fn = getattr(hip.lib(), name)  # and that is what the loaded library is called through
    assert (fn.restype, list(fn.argtypes)) == EXPECTED_SIGNATURES[name]


def test_void_pointer_out_parameters_take_what_the_call_sites_pass():
    from rec_pangu_amd import hip
    lib = hip.lib()
    n = ctypes.c_size_t(0)
    assert lib.rp_sort_workspace_bytes(1000, ctypes.byref(n)) == 0 and n.value > 0          # byref(...)
    buf, sec = ctypes.create_string_buffer(512), ctypes.c_int(0)
    assert lib.rp_plan_launch_name(None, 0, buf, 512, ctypes.byref(sec)) == -1               # a string buffer (no plan: refused)
    ints = (ctypes.c_int * 1)(3)
    assert lib.rp_ccpm_fits(3, 4, 1, ints, (ctypes.c_int * 1)(2), (ctypes.c_int * 1)(3)) == 1  # ctypes arrays
    with pytest.raises(ctypes.ArgumentError):  # (a bare c_size_t is not silently passed by value)
        lib.rp_sort_workspace_bytes(1000, n)


SYNTHETIC_HEADER = """
/* int rp_in_a_comment(int a); */
// int rp_in_a_line_comment(int a);
#include <stdint.h>
#define RP_SOME_CODE 0x30 /* hex */
#define RP_NEGATIVE (-3)
#define RP_NOT_AN_INTEGER "text"
#define OTHER_PREFIX 7
typedef void *rp_stream_t;
typedef struct {
    int64_t a, b;
    double c;
} rp_result;
#ifdef __cplusplus
extern "C" {
#endif
const char *rp_text(void);
uint64_t rp_count(void);
int64_t
rp_three_lines(const float *const *x_ptrs, int n, int32_t m, int64_t ld, uint32_t w, uint64_t bits, size_t bytes, float f,
               double d, rp_result *out, /* a comment between parameters */
               rp_stream_t stream);
#ifdef __cplusplus
}
#endif
"""


def test_parse_header_on_a_synthetic_header():
    from rec_pangu_amd.hip import parse_header
    sigs, consts = parse_header(SYNTHETIC_HEADER)
    assert list(sigs) == ["rp_text", "rp_count", "rp_three_lines"]  # header order; nothing from inside a comment
    assert sigs["rp_text"] == (ctypes.c_char_p, []) and sigs["rp_count"] == (ctypes.c_uint64, [])
    assert sigs["rp_three_lines"] == (ctypes.c_int64, [_vp, ctypes.c_int, ctypes.c_int, _i64, ctypes.c_uint32, _u64, _sz, _f32,
                                                       _f64, _vp, _vp])
    assert consts == {"RP_SOME_CODE": 0x30, "RP_NEGATIVE": -3}
    for bad, word in (("int rp_bad(long n);", "long"), ("int rp_bad(int n, unsigned int flags);", "unsigned"),
                      ("rp_result rp_bad(int n);", "rp_result"), ("float *rp_bad(int n);", "float"),
                      ("int rp_bad(int v[4]);", "v[4]"), ("static inline int rp_bad(int n) { return n; }", "rp_bad")):
        with pytest.raises(RuntimeError, match="rp_bad") as e:  # never a guess: the import fails and names the prototype
            parse_header(SYNTHETIC_HEADER + bad)
        assert word in str(e.value), (bad, str(e.value))


def test_constants_come_from_the_header_with_the_values_they_had():
    from rec_pangu_amd import hip
    assert (hip.ACT_NONE, hip.ACT_RELU, hip.ACT_MASK, hip.ACT_TANH, hip.ACT_SIGMOID, hip.ACT_LEAKY) == (0, 1, 2, 3, 4, 5)
    assert hip.MATMUL_MODES == {"fp32": 0, "bf16": 1, "auto": 2, "bf16x3": 3, "bf16x6": 6}
    assert hip.BILINEAR_TYPES == {"field_all": 0, "field_each": 1, "field_interaction": 2}
    assert (hip.METRIC_AUC, hip.METRIC_LOGLOSS) == (1, 2)
    assert hip.METRICS_STAGES == {"key": 0x100, "sort": 0x200, "tile_sums": 0x400, "tile_scan": 0x800, "group_neg": 0x1000,
                                  "rank": 0x2000, "finish": 0x4000}
    assert list(hip.METRICS_STAGES) == ["key", "sort", "tile_sums", "tile_scan", "group_neg", "rank", "finish"]  # issue order
    assert (hip.PAIR_ESSM, hip.PAIR_AITM) == (0, 1) and hip.POOL_MODES == {"sum": 0, "average": 1}
    assert hip.MAX_FIELDS == 64
    assert hip.ABI_VERSION == 108 == hip.lib().rp_version()


# ---- the one statement of the row-buffer contract (hip._rows) and of the padded width (functional.padded) --------------
def test_row_buffer_check_refuses_in_its_stated_order():
    import torch
    from rec_pangu_amd.hip import _rows
    B, cols = 4, 6

    def refused(t, word, B=B):
        with pytest.raises(RuntimeError, match=word) as e:
            _rows(t, "blk: x", cols, B)
        assert str(e.value).startswith("blk: x")

    # each tensor breaks the rule under test AND every later one: the earlier rule is the one reported
    refused(torch.zeros(3, 2, 8, dtype=torch.float64)[:, :, ::2], "float32")     # float32 first
    refused(torch.zeros(3, 2, 8)[:, :, ::2], "2-D")                              # then 2-D
    refused(torch.zeros(3, 8)[:, ::2], "unit inner stride")                      # then the inner stride (4 columns, 3 rows)
    refused(torch.zeros(3 * 5).as_strided((3, 5), (4, 1)), "narrower than 6")    # then the width (rows overlap, 3 rows)
    refused(torch.zeros(3 * 8).as_strided((3, 8), (5, 1)), "rows overlap.*narrower")  # then the overlap (3 rows)
    refused(torch.zeros(3, 8), "expected 4 rows")                                # the row count last
    refused(torch.zeros(B, cols, dtype=torch.float16), "float32")
    # what passes, and the leading dimension it returns
    assert _rows(torch.zeros(B, cols), "x", cols, B) == cols
    assert _rows(torch.zeros(B, 16)[:, :9], "x", cols, B) == 16                  # a wider buffer: its row stride
    assert _rows(torch.zeros(B, 16)[:, 3:9], "x", cols) == 16 and _rows(torch.zeros(7, cols), "x", cols) == cols  # B not given
    for stride in (0, 1, 5, 6, 100):                                            # one row: any row stride
        one = torch.zeros(128).as_strided((1, 8), (stride, 1))
        assert _rows(one, "x", cols, 1) == max(stride, 8)
    assert _rows(torch.zeros(0, 8), "x", cols, 0) == 8
    refused(torch.zeros(B * 8).as_strided((B, 8), (cols - 1, 1)), "narrower")    # wide enough, but the rows overlap


def test_parameter_list_check():
    import torch
    from rec_pangu_amd.hip import _params
    _params([("blk: W", torch.zeros(3, 4)), ("blk: b", torch.zeros(3))])
    with pytest.raises(RuntimeError, match=r"blk: b: expected torch.float32"):
        _params([("blk: W", torch.zeros(3, 4)), ("blk: b", torch.zeros(3).half())])
    with pytest.raises(RuntimeError, match="blk: W must be contiguous"):
        _params([("blk: W", torch.zeros(3, 8)[:, ::2]), ("blk: b", torch.zeros(3).half())])


def test_gin_rows_are_checked_like_its_siblings():
    """gin gained the overlap check and the host-before-device order of the ccpm / bilinear / lognet validators"""
    import torch
    from rec_pangu_amd import hip
    B, F, D, O = 4, 3, 8, 2
    x0, W, alpha, h = torch.zeros(B, F * D + 2), torch.zeros(O, D, D), torch.zeros(F * F, O), torch.zeros(O, D, 1)
    with pytest.raises(RuntimeError, match="float32"):
        hip.gin_fwd(x0.double(), x0.double(), W, alpha, h, F)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.gin_fwd(x0, x0, torch.zeros(O, D, 2 * D)[:, :, ::2], alpha, h, F)
    with pytest.raises(RuntimeError, match="narrower"):
        hip.gin_fwd(x0[:, :F * D - 1], x0, W, alpha, h, F)
    with pytest.raises(RuntimeError, match="narrower"):  # wide enough, but the rows overlap
        hip.gin_fwd(torch.zeros(B * F * D).as_strided((B, F * D), (F * D - 1, 1)), x0, W, alpha, h, F)
    with pytest.raises(RuntimeError, match="expected 4 rows"):
        hip.gin_fwd(x0, x0[:3], W, alpha, h, F)
    with pytest.raises(RuntimeError, match="narrower"):
        hip.gin_bwd(torch.zeros(B, O * D - 1), x0, x0, W, alpha, h, F, torch.zeros(B, F * D), False, bi_is_x0=True)
    with pytest.raises(RuntimeError, match="HIP-device"):  # every host-side check passed: only now the device matters
        hip.gin_fwd(x0, x0, W, alpha, h, F)
    with pytest.raises(RuntimeError, match="HIP-device"):
        hip.gin_bwd(torch.zeros(B, O * D), x0, x0, W, alpha, h, F, torch.zeros(B, F * D), False, bi_is_x0=True)


@pytest.mark.parametrize("pad_to", [1, 4, 64])
def test_padded_is_the_round_up_it_replaced(pad_to):
    from rec_pangu_amd.functional import padded
    for width in list(range(0, 3 * 64 + 2)) + [1677, 1680, 1728, 26 * 64 + 13]:  # exact multiples among them
        assert padded(width, pad_to) == (width + pad_to - 1) // pad_to * pad_to
        assert padded(width, pad_to) % pad_to == 0 and 0 <= padded(width, pad_to) - width < pad_to
    assert padded(1677, 0) == 1677 and padded(1677, -4) == 1677  # pad_to <= 1: the width itself
    assert padded(128, 64) == 128 and padded(129, 64) == 192 and padded(1677, 4) == 1680
