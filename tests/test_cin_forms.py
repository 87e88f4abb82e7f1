"""Which kernel form serves each layer of the compressed interaction network (functional.cin_forms), and the launches
the forms turn into (CompressedInteractionNet._forward_hip and the autograd functions behind it), both on the host.

FORMS is the table of the change that gathered the choice into cin_forms.  EXPECTED is the issue order: every hip entry
point on the path is replaced by a recorder that returns CPU tensors of the right shape, the module runs forward and
backward on CPU tensors with B = 8, and the ordered log of (entry point, H/M/O/D, want_out / want_pool, which gradients
are given, `into=` set or not, has_bias) is compared.  The literals in EXPECTED were recorded with this very recorder on
the code as it stood BEFORE the choice was gathered into one function; they are the specification, not a description of
the present code.  (The *_fits functions keep their library implementation, which needs no GPU, behind a counter.)"""
import pytest
import torch

from rec_pangu_amd import functional as Fh
from rec_pangu_amd import hip
from rec_pangu_amd.models.layers import CompressedInteractionNet

B = 8
PAIR, BS, F32 = ("pair",) * 3, ("bs",) * 3, ("f32",) * 3
CHUNKED, HEAD = ("chunked",) * 3, ("head", "last", "last")

# (H, D, units, precision, rows aligned) -> (X_0 made contiguous first, ((fwd, bwd_x, bwd_w) per layer)) or None
FORMS = {
    (26, 64, (128, 128), "auto", True): (False, (PAIR, HEAD)),
    (26, 64, (16, 16, 16), "auto", True): (False, (PAIR, CHUNKED, HEAD)),
    (26, 64, (16, 16, 16), "auto", False): (False, (("pair", "pair", "f32"), F32, HEAD)),
    (26, 64, (40, 70, 16), "auto", False): (True, (PAIR, CHUNKED, HEAD)),
    (26, 64, (136, 8), "auto", True): (False, (BS, HEAD)),
    (26, 64, (136, 8), "auto", False): (False, (("bs", "bs", "f32"), HEAD)),
    (26, 64, (16, 16, 16), "fp32", True): (False, (F32, F32, HEAD)),
    (16, 40, (8, 8), "auto", True): (False, (F32, HEAD)),
    (5, 8, (7,), "auto", True): (False, (("last",) * 3,)),
    (4, 80, (3,), "auto", True): (False, (("f32_1ch", "f32", "f32"),)),
    (26, 80, (40, 3), "auto", True): (False, (F32, ("f32_1ch", "f32", "f32"))),
    (26, 40, (40, 40, 8), "auto", True): None,
    (33, 64, (16, 16), "auto", True): None,
    (33, 8, (7,), "auto", True): None,
}


@pytest.mark.parametrize("key", list(FORMS), ids=lambda k: "H{}-D{}-{}-{}-{}".format(
    k[0], k[1], "_".join(map(str, k[2])), k[3], "aligned" if k[4] else "misaligned"))
def test_forms_table(key):
    H, D, units, precision, aligned = key
    plan = Fh.cin_forms(H, list(units), D, precision, aligned)
    if FORMS[key] is None:
        assert plan is None
        return
    assert (plan.x0_contiguous, tuple(tuple(f) for f in plan.layers)) == FORMS[key]


def test_forms_need_one_output_and_read_the_precision_in_force(monkeypatch):
    assert Fh.cin_forms(26, [128, 128], 64, "auto", True, n_outputs=2) is None
    monkeypatch.setattr(hip, "get_matmul_precision", lambda: "fp32")
    assert tuple(Fh.cin_forms(26, [16, 16], 64, None, True).layers[0]) == F32
    cin = CompressedInteractionNet(26, [40, 70, 16])
    assert not cin.hip_supported(26, 64)  # wide middle layers have no fp32 form
    monkeypatch.setattr(hip, "get_matmul_precision", lambda: "auto")
    assert cin.hip_supported(26, 64) and not cin.hip_supported(26, 40) and not cin.hip_supported(33, 64)


# ------------------------------------------------------------------------------------------------ the issue order
def _given(t) -> str:
    return "-" if t is None else "y"


class Recorder:
    """stands in for the hip entry points of the CIN path; `log` is the issue order"""
    LOGGED = ("cin_pair_pieces", "cin_pair_fwd", "cin_bs_fwd", "cin_layer_fwd", "bf16_pieces", "accumulate", "cin_pair_bwd_x",
              "cin_bs_bwd_x", "cin_pair_bwd_w", "cin_bs_bwd_w", "cin_layer_bwd_w", "cin_layer_bwd", "cin_last_fwd",
              "cin_last_bwd", "cin_head_params_fwd", "cin_head_params_bwd", "add_scalars", "sum_all", "add_rows_to",
              "linear_fwd", "linear_wgrad", "transpose", "multi_copy", "copy_rows_to", "zeros")
    FITS = ("cin_bs_fits", "cin_pair_fits", "cin_last_fits")

    def __init__(self, monkeypatch, precision: str, shifted_dxp: bool = False):
        self.log, self.fits_calls, self.shifted_dxp = [], 0, shifted_dxp
        for name in self.LOGGED:
            monkeypatch.setattr(hip, name, getattr(self, name))
        for name in self.FITS:
            monkeypatch.setattr(hip, name, self._counted(getattr(hip, name)))
        monkeypatch.setattr(hip, "get_matmul_precision", lambda: precision)

    def _counted(self, fn):
        def call(*a):
            self.fits_calls += 1
            return fn(*a)
        return call

    def _launch(self, name, **what):
        self.log.append(" ".join([name] + [f"{k}={v}" for k, v in what.items()]))

    @staticmethod
    def _outs(x0, O, D, want_out, want_pool):
        return (torch.zeros((x0.shape[0], O, D)) if want_out else None), (torch.zeros((x0.shape[0], O)) if want_pool else None)

    @staticmethod
    def _wgrad(shape, O, want_bias):
        return torch.zeros(shape), (torch.zeros(O) if want_bias else None)

    # ---- forward
    def cin_pair_pieces(self, W3, transposed=False, both=False):
        O, H = W3.shape[0], W3.shape[1]
        self._launch("cin_pair_pieces", H=H, O=O, both=int(both), transposed=int(transposed))
        npair = H * (H + 1) // 2
        wsp = torch.zeros((3, 128, (npair + 31) // 32 * 32), dtype=torch.bfloat16)
        wst = torch.zeros((3, (npair + 127) // 128 * 128, 128), dtype=torch.bfloat16)
        return (wsp, wst) if both else (wst if transposed else wsp)

    def bf16_pieces(self, w3):
        self._launch("bf16_pieces", shape="x".join(map(str, w3.shape)))
        return torch.zeros((w3.shape[0], 3, 32, 32), dtype=torch.bfloat16)

    def cin_pair_fwd(self, x0, wsp, bias, H, O, D, want_out, want_pool):
        self._launch("cin_pair_fwd", H=H, O=O, D=D, want_out=int(want_out), want_pool=int(want_pool),
                     has_bias=int(bias is not None))
        return self._outs(x0, O, D, want_out, want_pool)

    def cin_bs_fwd(self, x0, xp, wp, bias, H, M, O, D, want_out, want_pool):
        self._launch("cin_bs_fwd", H=H, M=M, O=O, D=D, want_out=int(want_out), want_pool=int(want_pool),
                     has_bias=int(bias is not None))
        return self._outs(x0, O, D, want_out, want_pool)

    def cin_layer_fwd(self, x0, xp, W, bias, H, M, D, want_out, want_pool):
        O = W.shape[0]
        self._launch("cin_layer_fwd", H=H, M=M, O=O, D=D, want_out=int(want_out), want_pool=int(want_pool),
                     has_bias=int(bias is not None), same=int(xp is x0))
        return self._outs(x0, O, D, want_out, want_pool)

    def accumulate(self, dst, src):
        self._launch("accumulate", shape="x".join(map(str, dst.shape)))
        return dst

    def cin_last_fwd(self, x0, xp, vt, H, M, D):
        self._launch("cin_last_fwd", H=H, M=M, D=D, same=int(xp is x0))
        return torch.zeros((x0.shape[0], 1))

    def cin_head_params_fwd(self, WL, bL, c, H, M):
        self._launch("cin_head_params_fwd", H=H, M=M, O=WL.shape[0], has_bias=int(bL is not None))
        return torch.zeros((M, 32)), torch.zeros(1)

    def add_scalars(self, out, a, scale, b0=None):
        self._launch("add_scalars", scale=scale, b0=_given(b0))
        return out

    def linear_fwd(self, a, w, bias, act=0, aux=None, K=None, out=None):
        self._launch("linear_fwd", N=w.shape[0], K=w.shape[1] if K is None else K, has_bias=int(bias is not None), act=act,
                     out=_given(out))
        return out if out is not None else torch.zeros((a.shape[0], w.shape[0]))

    # ---- backward
    def cin_pair_bwd_x(self, x0, wst, g_out, g_pool, H, O, D, like, into=None):
        self._launch("cin_pair_bwd_x", H=H, O=O, D=D, g_out=_given(g_out), g_pool=_given(g_pool), into=_given(into))
        return into if into is not None else torch.zeros_like(like)

    def cin_bs_bwd_x(self, xk, wp, g_out, g_pool, R, Cn, O, D, like, out=None):
        self._launch("cin_bs_bwd_x", R=R, C=Cn, O=O, D=D, g_out=_given(g_out), g_pool=_given(g_pool), like=_given(like),
                     out=_given(out))
        return out if out is not None else torch.zeros_like(like)

    def cin_pair_bwd_w(self, x0, g_out, g_pool, H, O, D, want_bias):
        self._launch("cin_pair_bwd_w", H=H, O=O, D=D, g_out=_given(g_out), g_pool=_given(g_pool), has_bias=int(want_bias))
        return self._wgrad((O, H * H), O, want_bias)

    def cin_bs_bwd_w(self, x0, xp, g_out, g_pool, H, M, O, D, want_bias):
        self._launch("cin_bs_bwd_w", H=H, M=M, O=O, D=D, g_out=_given(g_out), g_pool=_given(g_pool), has_bias=int(want_bias),
                     same=int(xp is x0))
        return self._wgrad((O, H * M), O, want_bias)

    def cin_layer_bwd_w(self, x0, xp, W, H, M, D, g_out, g_pool, want_bias):
        self._launch("cin_layer_bwd_w", H=H, M=M, O=W.shape[0], D=D, g_out=_given(g_out), g_pool=_given(g_pool),
                     has_bias=int(want_bias), same=int(xp is x0))
        return self._wgrad(W.shape, W.shape[0], want_bias)

    def cin_layer_bwd(self, x0, xp, W, H, M, D, g_out, g_pool, want_bias):
        self._launch("cin_layer_bwd", H=H, M=M, O=W.shape[0], D=D, g_out=_given(g_out), g_pool=_given(g_pool),
                     has_bias=int(want_bias), same=int(xp is x0))
        dxp = None if xp is x0 else torch.zeros((x0.shape[0], M * D))
        return (torch.zeros_like(x0), dxp) + self._wgrad(W.shape, W.shape[0], want_bias)

    def cin_last_bwd(self, x0, xp, vt, g, H, M, D):
        self._launch("cin_last_bwd", H=H, M=M, D=D, same=int(xp is x0))
        dxp = torch.zeros_like(xp)
        if self.shifted_dxp:  # contiguous, one float into a larger buffer: not 16-byte aligned
            dxp = torch.zeros(xp.numel() + 1)[1:].view(xp.shape)
            assert dxp.is_contiguous() and dxp.data_ptr() % 16 == 4
        return torch.zeros_like(x0), dxp, torch.zeros((H, M))

    def sum_all(self, x):
        self._launch("sum_all")
        return torch.zeros(1)

    def cin_head_params_bwd(self, WL, bL, c, dV, sg, D, H, M):
        O = WL.shape[0]
        self._launch("cin_head_params_bwd", H=H, M=M, O=O, D=D, has_bias=int(bL is not None))
        return torch.zeros((O, H * M)), (torch.zeros(O) if bL is not None else None), torch.zeros(O)

    def add_rows_to(self, src, dst):
        self._launch("add_rows_to", cols=src.shape[1])
        return dst

    def transpose(self, w, rows_out=None):
        self._launch("transpose")
        return torch.zeros((rows_out or w.shape[1], w.shape[0]))

    def linear_wgrad(self, dy, x, K, dw=None, db=None, accumulate=False, want_bias=True):
        self._launch("linear_wgrad", N=dy.shape[1], K=K, has_bias=int(want_bias))
        return torch.zeros((dy.shape[1], K)), (torch.zeros(dy.shape[1]) if want_bias else None)

    def multi_copy(self, dst, src):
        self._launch("multi_copy", n=len(dst))
        return True

    def copy_rows_to(self, src, dst):
        self._launch("copy_rows_to")

    def zeros(self, shape, dtype, device):
        self._launch("zeros")
        return torch.zeros(shape, dtype=dtype)


def _run(monkeypatch, H, D, units, precision="auto", aligned=True, shifted_dxp=False):
    rec = Recorder(monkeypatch, precision, shifted_dxp)
    torch.manual_seed(0)
    cin = CompressedInteractionNet(H, list(units), output_dim=1)
    ld = H * D + (0 if aligned else 13)  # misaligned rows: a [B, H*D + 13] buffer, as test_cin_vs_oracle builds one
    xbuf = torch.zeros((B, ld), requires_grad=True)
    out = cin._forward_hip(xbuf[:, :H * D].unflatten(1, (H, D)))
    assert out.shape == (B, 1)
    rec.log.append("backward")
    n_fits = rec.fits_calls
    out.sum().backward()
    assert rec.fits_calls == n_fits  # the backward decides nothing: it reads its forms from the forward
    assert xbuf.grad is not None and all(p.grad is not None for p in cin.parameters())
    return rec.log


CASES = [(26, 64, (128, 128), "auto", True), (26, 64, (16, 16, 16), "auto", True), (26, 64, (16, 16, 16), "auto", False),
         (26, 64, (40, 70, 16), "auto", False), (26, 64, (136, 8), "auto", True), (26, 64, (136, 8), "auto", False),
         (26, 64, (16, 16, 16), "fp32", True), (16, 40, (8, 8), "auto", True), (5, 8, (7,), "auto", True),
         (4, 80, (3,), "auto", True)]

# recorded on the parent of the change that gathered the choice into functional.cin_forms (see the module docstring)
EXPECTED = {
    (26, 64, (128, 128), 'auto', True): [
        'cin_pair_pieces H=26 O=128 both=1 transposed=0',
        'cin_pair_fwd H=26 O=128 D=64 want_out=1 want_pool=1 has_bias=1',
        'cin_head_params_fwd H=26 M=128 O=128 has_bias=1',
        'cin_last_fwd H=26 M=128 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=128 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=128 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=128 has_bias=0',
        'cin_last_bwd H=26 M=128 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=128 O=128 D=64 has_bias=1',
        'multi_copy n=2',
        'cin_pair_bwd_x H=26 O=128 D=64 g_out=y g_pool=y into=y',
        'cin_pair_bwd_w H=26 O=128 D=64 g_out=y g_pool=y has_bias=1',
    ],
    (26, 64, (16, 16, 16), 'auto', True): [
        'cin_pair_pieces H=26 O=16 both=1 transposed=0',
        'cin_pair_fwd H=26 O=16 D=64 want_out=1 want_pool=1 has_bias=1',
        'bf16_pieces shape=16x26x16',
        'cin_bs_fwd H=26 M=16 O=16 D=64 want_out=1 want_pool=1 has_bias=1',
        'cin_head_params_fwd H=26 M=16 O=16 has_bias=1',
        'cin_last_fwd H=26 M=16 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=32 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=32 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=32 has_bias=0',
        'cin_last_bwd H=26 M=16 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=16 O=16 D=64 has_bias=1',
        'multi_copy n=2',
        'bf16_pieces shape=16x26x16',
        'cin_bs_bwd_x R=26 C=16 O=16 D=64 g_out=y g_pool=y like=y out=-',
        'bf16_pieces shape=16x16x26',
        'cin_bs_bwd_x R=16 C=26 O=16 D=64 g_out=y g_pool=y like=- out=y',
        'cin_bs_bwd_w H=26 M=16 O=16 D=64 g_out=y g_pool=y has_bias=1 same=0',
        'cin_pair_bwd_x H=26 O=16 D=64 g_out=y g_pool=y into=y',
        'cin_pair_bwd_w H=26 O=16 D=64 g_out=y g_pool=y has_bias=1',
    ],
    (26, 64, (16, 16, 16), 'auto', False): [
        'cin_pair_pieces H=26 O=16 both=1 transposed=0',
        'cin_pair_fwd H=26 O=16 D=64 want_out=1 want_pool=1 has_bias=1',
        'cin_layer_fwd H=26 M=16 O=16 D=64 want_out=1 want_pool=1 has_bias=1 same=0',
        'cin_head_params_fwd H=26 M=16 O=16 has_bias=1',
        'cin_last_fwd H=26 M=16 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=32 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=32 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=32 has_bias=0',
        'cin_last_bwd H=26 M=16 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=16 O=16 D=64 has_bias=1',
        'multi_copy n=2',
        'cin_layer_bwd H=26 M=16 O=16 D=64 g_out=y g_pool=y has_bias=1 same=0',
        'cin_pair_bwd_x H=26 O=16 D=64 g_out=y g_pool=y into=y',
        'cin_layer_bwd_w H=26 M=26 O=16 D=64 g_out=y g_pool=y has_bias=1 same=1',
    ],
    (26, 64, (40, 70, 16), 'auto', False): [
        'cin_pair_pieces H=26 O=40 both=1 transposed=0',
        'cin_pair_fwd H=26 O=40 D=64 want_out=1 want_pool=1 has_bias=1',
        'bf16_pieces shape=70x26x32',
        'cin_bs_fwd H=26 M=32 O=70 D=64 want_out=1 want_pool=1 has_bias=1',
        'bf16_pieces shape=70x26x8',
        'cin_bs_fwd H=26 M=8 O=70 D=64 want_out=1 want_pool=1 has_bias=0',
        'accumulate shape=8x70x64',
        'accumulate shape=8x70',
        'cin_head_params_fwd H=26 M=70 O=16 has_bias=1',
        'cin_last_fwd H=26 M=70 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=110 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=110 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=110 has_bias=0',
        'cin_last_bwd H=26 M=70 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=70 O=16 D=64 has_bias=1',
        'multi_copy n=2',
        'bf16_pieces shape=70x26x32',
        'cin_bs_bwd_x R=26 C=32 O=70 D=64 g_out=y g_pool=y like=y out=-',
        'bf16_pieces shape=70x32x26',
        'cin_bs_bwd_x R=32 C=26 O=70 D=64 g_out=y g_pool=y like=- out=y',
        'cin_bs_bwd_w H=26 M=32 O=70 D=64 g_out=y g_pool=y has_bias=1 same=0',
        'bf16_pieces shape=70x26x8',
        'cin_bs_bwd_x R=26 C=8 O=70 D=64 g_out=y g_pool=y like=y out=-',
        'accumulate shape=8x1664',
        'bf16_pieces shape=70x8x26',
        'cin_bs_bwd_x R=8 C=26 O=70 D=64 g_out=y g_pool=y like=- out=y',
        'cin_bs_bwd_w H=26 M=8 O=70 D=64 g_out=y g_pool=y has_bias=0 same=0',
        'cin_pair_bwd_x H=26 O=40 D=64 g_out=y g_pool=y into=y',
        'cin_pair_bwd_w H=26 O=40 D=64 g_out=y g_pool=y has_bias=1',
    ],
    (26, 64, (136, 8), 'auto', True): [
        'bf16_pieces shape=136x26x26',
        'cin_bs_fwd H=26 M=26 O=136 D=64 want_out=1 want_pool=1 has_bias=1',
        'cin_head_params_fwd H=26 M=136 O=8 has_bias=1',
        'cin_last_fwd H=26 M=136 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=136 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=136 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=136 has_bias=0',
        'cin_last_bwd H=26 M=136 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=136 O=8 D=64 has_bias=1',
        'multi_copy n=2',
        'bf16_pieces shape=136x26x26',
        'cin_bs_bwd_x R=26 C=26 O=136 D=64 g_out=y g_pool=y like=y out=-',
        'add_rows_to cols=1664',
        'cin_bs_bwd_w H=26 M=26 O=136 D=64 g_out=y g_pool=y has_bias=1 same=1',
    ],
    (26, 64, (136, 8), 'auto', False): [
        'bf16_pieces shape=136x26x26',
        'cin_bs_fwd H=26 M=26 O=136 D=64 want_out=1 want_pool=1 has_bias=1',
        'cin_head_params_fwd H=26 M=136 O=8 has_bias=1',
        'cin_last_fwd H=26 M=136 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=136 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=136 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=136 has_bias=0',
        'cin_last_bwd H=26 M=136 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=136 O=8 D=64 has_bias=1',
        'multi_copy n=2',
        'bf16_pieces shape=136x26x26',
        'cin_bs_bwd_x R=26 C=26 O=136 D=64 g_out=y g_pool=y like=y out=-',
        'add_rows_to cols=1664',
        'cin_layer_bwd_w H=26 M=26 O=136 D=64 g_out=y g_pool=y has_bias=1 same=1',
    ],
    (26, 64, (16, 16, 16), 'fp32', True): [
        'cin_layer_fwd H=26 M=26 O=16 D=64 want_out=1 want_pool=1 has_bias=1 same=1',
        'cin_layer_fwd H=26 M=16 O=16 D=64 want_out=1 want_pool=1 has_bias=1 same=0',
        'cin_head_params_fwd H=26 M=16 O=16 has_bias=1',
        'cin_last_fwd H=26 M=16 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=32 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=32 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=32 has_bias=0',
        'cin_last_bwd H=26 M=16 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=16 O=16 D=64 has_bias=1',
        'multi_copy n=2',
        'cin_layer_bwd H=26 M=16 O=16 D=64 g_out=y g_pool=y has_bias=1 same=0',
        'cin_layer_bwd H=26 M=26 O=16 D=64 g_out=y g_pool=y has_bias=1 same=1',
        'add_rows_to cols=1664',
    ],
    (16, 40, (8, 8), 'auto', True): [
        'cin_layer_fwd H=16 M=16 O=8 D=40 want_out=1 want_pool=1 has_bias=1 same=1',
        'cin_head_params_fwd H=16 M=8 O=8 has_bias=1',
        'cin_last_fwd H=16 M=8 D=40 same=0',
        'add_scalars scale=40.0 b0=y',
        'linear_fwd N=1 K=8 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=8 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=8 has_bias=0',
        'cin_last_bwd H=16 M=8 D=40 same=0',
        'sum_all',
        'cin_head_params_bwd H=16 M=8 O=8 D=40 has_bias=1',
        'multi_copy n=2',
        'cin_layer_bwd H=16 M=16 O=8 D=40 g_out=y g_pool=y has_bias=1 same=1',
        'add_rows_to cols=640',
    ],
    (5, 8, (7,), 'auto', True): [
        'cin_last_fwd H=5 M=5 D=8 same=1',
        'backward',
        'cin_last_bwd H=5 M=5 D=8 same=1',
    ],
    (4, 80, (3,), 'auto', True): [
        'cin_layer_fwd H=4 M=4 O=1 D=80 want_out=0 want_pool=1 has_bias=1 same=1',
        'backward',
        'cin_layer_bwd H=4 M=4 O=1 D=80 g_out=- g_pool=y has_bias=1 same=1',
    ],
    (26, 64, (128, 128), 'auto', True, 'g_out misaligned'): [
        'cin_pair_pieces H=26 O=128 both=1 transposed=0',
        'cin_pair_fwd H=26 O=128 D=64 want_out=1 want_pool=1 has_bias=1',
        'cin_head_params_fwd H=26 M=128 O=128 has_bias=1',
        'cin_last_fwd H=26 M=128 D=64 same=0',
        'add_scalars scale=64.0 b0=y',
        'linear_fwd N=1 K=128 has_bias=0 act=0 out=-',
        'backward',
        'transpose',
        'linear_fwd N=128 K=1 has_bias=0 act=0 out=y',
        'linear_wgrad N=1 K=128 has_bias=0',
        'cin_last_bwd H=26 M=128 D=64 same=0',
        'sum_all',
        'cin_head_params_bwd H=26 M=128 O=128 D=64 has_bias=1',
        'multi_copy n=2',
        'bf16_pieces shape=128x26x26',
        'cin_bs_bwd_x R=26 C=26 O=128 D=64 g_out=y g_pool=y like=y out=-',
        'add_rows_to cols=1664',
        'cin_pair_bwd_w H=26 O=128 D=64 g_out=y g_pool=y has_bias=1',
    ],
}


@pytest.mark.parametrize("H,D,units,precision,aligned", CASES)
def test_issue_order(monkeypatch, H, D, units, precision, aligned):
    assert _run(monkeypatch, H, D, units, precision, aligned) == EXPECTED[H, D, units, precision, aligned]


def test_issue_order_with_a_misaligned_output_gradient(monkeypatch):
    """the one run-time exception: the pair form's gradient of X_0 reads g_out with 16-byte loads, so a g_out that is not
    16-byte aligned (here: the collapsed last layer's gradient of X_1, one float into a larger buffer) takes the per-channel
    form for that one launch; the weight gradient stays in the pair form"""
    log = _run(monkeypatch, 26, 64, (128, 128), shifted_dxp=True)
    assert log == EXPECTED[26, 64, (128, 128), "auto", True, "g_out misaligned"]
    assert any(e.startswith("cin_bs_bwd_x") for e in log) and not any(e.startswith("cin_pair_bwd_x") for e in log)
