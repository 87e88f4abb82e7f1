"""The fused MLP tail (csrc/mlp_tail.hip) through the C ABI at the edges of its decomposition: a workgroup takes 128 rows,
a wave 32 of them, the weight gradient contracts over the workgroup's rows in k-steps of 16, per-workgroup partials are
summed by a second launch.  Every case: seeded inputs, an fp64 autograd reference built as in test_mlp_tail_fused_vs_fp64, that
test's tolerance (2e-5 of each gradient's scale; logits and activations rtol 1e-5 / atol 2e-5)."""
import ctypes as C

import pytest
import torch

from conftest import require_gpu

pytestmark = pytest.mark.gpu

DEV = "cuda"
CANARY = -1.0e30


@pytest.fixture(scope="module")
def hip():
    require_gpu()
    from rec_pangu_amd import hip as h
    h.lib()
    return h


def _per(L):
    return L * 4096 + L * 64 + 65


class Problem:
    """One seeded tail problem and its fp64 reference (computed once per instance)."""

    def __init__(self, M, L, seed, steer=False):
        g = torch.Generator().manual_seed(seed)
        pre = torch.randn(M, 64, generator=g)
        self.Ws = [torch.randn(64, 64, generator=g) / 8 for _ in range(L)]
        self.bs = [torch.randn(64, generator=g) * 0.1 for _ in range(L)]
        self.zero_rows = {}
        if steer:
            # rows whose input, second or third hidden output is exactly zero in EVERY column: one strong input feature is
            # routed to one unit of a layer, and the next layer's weights from that unit are all -1
            assert L == 3 and M >= 12
            r_in, r_h2, r_h3 = [0, M // 2, M - 1], [1, M // 2 + 1, M - 2], [2, M // 2 + 2, M - 3]
            pre[r_in] = -pre[r_in].abs() - 0.5           # hin rows = 0
            pre[r_h2, 0] = 50.0
            self.Ws[0][7, 0] = 1.0                       # h1[:, 7] ~ 50 ...
            self.Ws[1][:, 7] = -1.0                      # ... pushes every h2 pre-activation of those rows below zero
            pre[r_h3, 1] = 50.0
            self.Ws[0][9, 1] = 1.0
            self.Ws[1][11, 9] = 1.0                      # h2[:, 11] ~ 50
            self.Ws[2][:, 11] = -1.0                     # every h3 pre-activation of those rows below zero
            self.zero_rows = {0: r_in, 2: r_h2, 3: r_h3}
        self.M, self.L = M, L
        self.hin = pre.relu()                            # the tail's input is a ReLU output
        self.w_out = torch.randn(1, 64, generator=g) / 8
        self.b_out = torch.randn(1, generator=g)
        self.dz = torch.randn(M, generator=g) / M
        p64 = pre.double().requires_grad_(True)
        W64 = [w.double().requires_grad_(True) for w in self.Ws]
        b64 = [b.double().requires_grad_(True) for b in self.bs]
        wo64, bo64 = self.w_out.double().requires_grad_(True), self.b_out.double().requires_grad_(True)
        a = p64.relu()
        acts = []
        for w, b in zip(W64, b64):
            a = (a @ w.t() + b).relu()
            acts.append(a)
        logit = a @ wo64.t() + bo64
        (logit.reshape(-1) * self.dz.double()).sum().backward()
        self.ref_logit, self.ref_acts = logit.detach(), [t.detach() for t in acts]
        self.ref = {"dhin": p64.grad, "dW": [w.grad for w in W64], "db": [b.grad for b in b64], "dwo": wo64.grad, "dbo": bo64.grad}


class Device:
    """The problem's tensors on the device, laid out with the given row strides, and the C-ABI calls on them."""

    def __init__(self, hip, p, ld0=64, lddh=64, pad_rows=0):
        self.hip, self.p, self.lddh, self.ld0 = hip, p, lddh, ld0
        M, L = p.M, p.L
        buf = torch.full((M + pad_rows, ld0), CANARY)
        buf[:M, :64] = p.hin
        self.hin_buf = buf.to(DEV)
        self.hin_host = buf
        self.Ws = [w.to(DEV) for w in p.Ws]
        self.bs = [b.to(DEV) for b in p.bs]
        self.w_out, self.b_out, self.dz = p.w_out.to(DEV), p.b_out.to(DEV), p.dz.to(DEV)
        self.hs = [torch.empty(M, 64, device=DEV) for _ in range(L)]
        self.logit = torch.empty(M, 1, device=DEV)
        self.pad_rows = pad_rows
        nbytes = C.c_size_t(0)
        assert hip.lib().rp_mlp_tail_bwd_workspace_bytes(M, L, C.byref(nbytes)) == 0
        self.nbytes = nbytes.value
        self.ws = torch.zeros(self.nbytes, dtype=torch.uint8, device=DEV)

    def fwd(self):
        hip, L = self.hip, self.p.L
        rc = hip.lib().rp_mlp_tail_fwd(self.hin_buf.data_ptr(), self.ld0, L, hip._ptr_array(self.Ws), hip._i64_array([64] * L),
                                       hip._opt_ptr_array(self.bs), hip._ptr_array(self.hs), self.w_out.data_ptr(),
                                       self.b_out.data_ptr(), self.logit.data_ptr(), self.p.M, hip._stream())
        assert rc == 0
        return self.logit, self.hs

    def new_outputs(self):
        dhin = torch.full((self.p.M + self.pad_rows, self.lddh), CANARY, device=DEV)
        grads = torch.full((_per(self.p.L),), CANARY, device=DEV)
        return dhin, grads

    def bwd(self, parts_seq=(3,), dz=None, ws=None):
        """-> (dhin buffer [M + pad, lddh], grads) after rp_mlp_tail_bwd_parts for every entry of parts_seq"""
        hip, L = self.hip, self.p.L
        dhin, grads = self.new_outputs()
        dz = self.dz if dz is None else dz
        ws = self.ws if ws is None else ws
        acts = [self.hin_buf] + self.hs
        for parts in parts_seq:
            rc = hip.lib().rp_mlp_tail_bwd_parts(dz.data_ptr(), L, hip._ptr_array(self.Ws), hip._i64_array([64] * L),
                                                 hip._ptr_array(acts), self.ld0, self.w_out.data_ptr(), dhin.data_ptr(), self.lddh,
                                                 grads.data_ptr(), self.p.M, ws.data_ptr(), self.nbytes, parts, hip._stream())
            assert rc == 0
        return dhin, grads


def _close(got, ref, what):
    scale = float(ref.abs().max())
    err = float((got.cpu().double() - ref).abs().max())
    print(f"{what}: err {err:.3e} scale {scale:.3e} ratio {err / max(scale, 1e-12):.2e}")
    assert err <= 2e-5 * max(scale, 1e-12), f"{what}: {err} vs scale {scale}"


def _check_against_fp64(p, dhin_buf, grads):
    M, L = p.M, p.L
    _close(dhin_buf[:M, :64], p.ref["dhin"], "d hin (masked)")
    for l in range(L):
        _close(grads[l * 4096:(l + 1) * 4096].view(64, 64), p.ref["dW"][l], f"dW{l}")
        _close(grads[L * 4096 + l * 64:L * 4096 + (l + 1) * 64], p.ref["db"][l], f"db{l}")
    _close(grads[L * 4160:L * 4160 + 64].view(1, 64), p.ref["dwo"], "dw_out")
    _close(grads[L * 4160 + 64:L * 4160 + 65], p.ref["dbo"], "db_out")
    assert bool((dhin_buf[:M, :64].cpu()[p.hin == 0] == 0).all()), "a masked entry of dhin is not exactly 0.0"


def _check_forward(p, logit, hs):
    torch.testing.assert_close(logit.cpu().double(), p.ref_logit, rtol=1e-5, atol=2e-5)
    for got, ref in zip(hs, p.ref_acts):
        torch.testing.assert_close(got.cpu().double(), ref, rtol=1e-5, atol=2e-5)


# one below, at and one above: the wgrad's k-step (16 rows), a wave's rows (32), two and three waves, a workgroup (128), two
# workgroups and one row
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257])
def test_every_tile_edge_vs_fp64(hip, M, L):
    p = Problem(M, L, seed=1000 * L + M)
    d = Device(hip, p)
    _check_forward(p, *d.fwd())
    dhin, grads = d.bwd()
    _check_against_fp64(p, dhin, grads)


@pytest.mark.parametrize("M,L,ld0,lddh", [(129, 2, 68, 64), (129, 2, 64, 68), (257, 3, 128, 128), (33, 1, 68, 72)])
def test_row_strides_and_untouched_padding(hip, M, L, ld0, lddh):
    """hin with a row stride above 64 and dhin with lddh above 64: the columns beyond 64 and the rows past M hold a canary
    that the launches neither use nor overwrite"""
    p = Problem(M, L, seed=77 * M + L)
    d = Device(hip, p, ld0=ld0, lddh=lddh, pad_rows=5)
    _check_forward(p, *d.fwd())
    dhin, grads = d.bwd()
    _check_against_fp64(p, dhin, grads)
    assert bool((dhin[M:] == CANARY).all()), "rows of dhin past M were written"
    assert bool((dhin[:, 64:] == CANARY).all()), "columns of dhin beyond 64 were written"
    assert torch.equal(d.hin_buf.cpu(), d.hin_host), "the input buffer changed"


def test_rows_that_are_zero_at_every_level(hip):
    """whole rows of hin, of h2 and of h3 exactly zero (the reference agrees that they are), and single zeros everywhere
    else: gradients against fp64, masked entries of dhin exactly 0.0"""
    M, L = 200, 3
    p = Problem(M, L, seed=4242, steer=True)
    assert bool((p.hin[p.zero_rows[0]] == 0).all())
    assert bool((p.ref_acts[1][p.zero_rows[2]] == 0).all()) and bool((p.ref_acts[0][p.zero_rows[2]] > 0).any())
    assert bool((p.ref_acts[2][p.zero_rows[3]] == 0).all()) and bool((p.ref_acts[1][p.zero_rows[3]] > 0).any())
    d = Device(hip, p)
    logit, hs = d.fwd()
    _check_forward(p, logit, hs)
    assert bool((hs[1][p.zero_rows[2]] == 0).all()) and bool((hs[2][p.zero_rows[3]] == 0).all())
    dhin, grads = d.bwd()
    _check_against_fp64(p, dhin, grads)
    assert bool((dhin[p.zero_rows[0]] == 0).all())
    assert bool((dhin[p.zero_rows[3]] == 0).all()), "no gradient passes a row whose last hidden output is all zero"


def test_single_zero_activations(hip):
    """about half of every activation is exactly 0.0 (plain ReLU outputs), none of the rows is: the mask per element"""
    p = Problem(300, 2, seed=99)
    assert 0.3 < float((p.hin == 0).float().mean()) < 0.7 and bool((p.hin > 0).any(dim=1).all())
    d = Device(hip, p)
    _check_forward(p, *d.fwd())
    dhin, grads = d.bwd()
    _check_against_fp64(p, dhin, grads)


@pytest.mark.parametrize("M,L", [(129, 2), (4099, 2), (4099, 3), (129, 1), (16385, 2)])
def test_parts_compose_and_repeat_bitwise(hip, M, L):
    """two, 33 and 129 workgroups (from 113 on the second stage takes its eight-at-a-time loop): parts 1 then 2 = parts 3,
    and two full launches agree bit for bit"""
    p = Problem(M, L, seed=31 * M + L)
    d = Device(hip, p)
    d.fwd()
    a = d.bwd((3,))
    b = d.bwd((1, 2), ws=torch.zeros_like(d.ws))
    c = d.bwd((3,))
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y), "parts 1 then 2 differ from parts 3"
        assert torch.equal(x, z), "two launches differ"
    _check_against_fp64(p, *a)


@pytest.mark.parametrize("ld0,lddh", [(64, 64), (68, 72)])
def test_fused_bce_entry_equals_dz_entry(hip, ld0, lddh):
    """rp_mlp_tail_bwd_bce at M = 129, L = 2, one other logit addend, with and without padded rows: its dz_out, fed to the dz
    entry, gives the same bits"""
    M, L = 129, 2
    p = Problem(M, L, seed=555)
    d = Device(hip, p, ld0=ld0, lddh=lddh, pad_rows=3)
    g = torch.Generator().manual_seed(556)
    add = torch.randn(M, generator=g).to(DEV)
    label = (torch.rand(M, generator=g) < 0.3).float().to(DEV)
    gloss = torch.tensor([0.75], device=DEV)
    pred = torch.empty(M, device=DEV)
    partial = torch.empty(hip.lib().rp_mlp_tail_loss_partials(M), device=DEV)
    lib = hip.lib()
    rc = lib.rp_mlp_tail_fwd_bce(d.hin_buf.data_ptr(), ld0, L, hip._ptr_array(d.Ws), hip._i64_array([64] * L), hip._opt_ptr_array(d.bs),
                                 hip._ptr_array(d.hs), d.w_out.data_ptr(), d.b_out.data_ptr(), hip._ptr_array([add]), 1,
                                 label.data_ptr(), 0.0, pred.data_ptr(), partial.data_ptr(), M, hip._stream())
    assert rc == 0
    # pred against the reference's logit + addend
    z = p.ref_logit.reshape(-1) + add.cpu().double()
    torch.testing.assert_close(pred.cpu().double(), torch.sigmoid(z), rtol=1e-5, atol=2e-5)
    dz_out = torch.full((M,), CANARY, device=DEV)
    dhin, grads = d.new_outputs()
    acts = [d.hin_buf] + d.hs
    rc = lib.rp_mlp_tail_bwd_bce(pred.data_ptr(), label.data_ptr(), gloss.data_ptr(), 0.0, 1.0, dz_out.data_ptr(), L,
                                 hip._ptr_array(d.Ws), hip._i64_array([64] * L), hip._ptr_array(acts), ld0, d.w_out.data_ptr(),
                                 dhin.data_ptr(), lddh, grads.data_ptr(), M, d.ws.data_ptr(), d.nbytes, 3, hip._stream())
    assert rc == 0
    # dz_out against the closed form of the sigmoid + BCE gradient: (pred - label) * gloss / M
    ref_dz = (pred.cpu().double() - label.cpu().double()) * 0.75 / M
    _close(dz_out, ref_dz, "dz_out")
    dhin2, grads2 = d.bwd((3,), dz=dz_out, ws=torch.zeros_like(d.ws))
    assert torch.equal(dhin, dhin2), "dhin differs between the two entries"
    assert torch.equal(grads, grads2), "gradients differ between the two entries"
    assert bool((dhin[M:] == CANARY).all()) and bool((dhin[:, 64:] == CANARY).all()), "dhin's padding was written"


# the second stage adds one workgroup at a time up to 112 workgroups and takes eight per lane and iteration from 113 on
# (slice q enters that loop when q + 112 < nwg: slice 0 alone at 113, every slice from 128): one below, at and above both,
# a remainder behind the loop (129, 145), two iterations (257) and the benchmark's 512
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("nwg", [1, 2, 15, 16, 17, 33, 112, 113, 127, 128, 129, 145, 257, 512])
def test_second_stage_alone_sums_in_the_documented_order(hip, nwg, L):
    """random partials in the workspace, parts = 2 alone: out[e] is the float32 sum over the workgroups in 16 interleaved
    slices (slice q: g = q, q + 16, ..), then the 16 slice sums in order — bit for bit"""
    M, per = nwg * 128 - 5, _per(L)
    lib = hip.lib()
    nbytes = C.c_size_t(0)
    assert lib.rp_mlp_tail_bwd_workspace_bytes(M, L, C.byref(nbytes)) == 0
    g = torch.Generator().manual_seed(9 * nwg + L)
    P = torch.randn(nwg, per, generator=g) * torch.logspace(-3, 3, nwg).reshape(-1, 1)
    ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=DEV)
    off = (-ws.data_ptr()) % 256  # the partials start at the workspace's first 256-byte boundary
    ws[off:off + nwg * per * 4] = P.reshape(-1).view(torch.uint8).to(DEV)
    # the second stage reads nothing but the workspace: the other arguments only have to be valid
    Ws = [torch.zeros(64, 64, device=DEV) for _ in range(L)]
    acts = [torch.zeros(M, 64, device=DEV) for _ in range(L + 1)]
    dz, w_out = torch.zeros(M, device=DEV), torch.zeros(1, 64, device=DEV)
    dhin = torch.full((M, 64), CANARY, device=DEV)
    grads = torch.full((per,), CANARY, device=DEV)
    rc = lib.rp_mlp_tail_bwd_parts(dz.data_ptr(), L, hip._ptr_array(Ws), hip._i64_array([64] * L), hip._ptr_array(acts), 64,
                                   w_out.data_ptr(), dhin.data_ptr(), 64, grads.data_ptr(), M, ws.data_ptr(), nbytes.value, 2,
                                   hip._stream())
    assert rc == 0
    slices = []
    for q in range(16):
        s = torch.zeros(per)
        for gi in range(q, nwg, 16):
            s = s + P[gi]
        slices.append(s)
    tot = slices[0]
    for j in range(1, 16):
        tot = tot + slices[j]
    assert torch.equal(grads.cpu(), tot)
    assert bool((dhin == CANARY).all()), "the second stage alone wrote dhin"
