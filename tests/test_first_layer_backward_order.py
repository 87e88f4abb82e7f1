"""The issue order of the fused lookup + first Linear's backward (functional._EmbedGatherLinear.backward and the
EmbeddingLayer methods it drives): which launches, in which order, on which plan section, with which field masks.  The GPU
tests compare results, which a launch on the wrong section usually leaves intact; this one pins the sequence itself, on
the host: every hip entry point on the path and LaunchPlan's section calls are replaced by recorders, the layer is a CPU
EmbeddingLayer with D = 64 and the sort is a hand-made SortedLookup.  (functional._wgrad_stream is stubbed to None: the
second-torch-stream variant of the eager loop is the one thing not seen here.)

The literals in EXPECTED were recorded with this very recorder on the code as it stood BEFORE the backward was gathered
into one function; they are the specification, not a description of the present code.  `held=1 / 0` (whether the launch
ran inside a hip.holding() block, which keeps what it allocates until the block ends) stands where that recording had
`keep=plan / None`; it is 1 for EVERY launch between the point a recording backward opens its block and the plan's join."""
from types import SimpleNamespace

import pytest
import torch

from rec_pangu_amd import functional as Fh
from rec_pangu_amd import hip
from rec_pangu_amd.models.layers import embedding as E

B = 512
ND = 13  # dense columns behind the embedding columns of the first Linear
# rows per table; with B = 512: tiny = at most 254 rows (two or more of them), big = at least B rows, mid = the rest
TABLES = {
    "tiny+big+mid": [600, 5, 300, 3, 7, 1000],  # tiny 1, 3, 4; big 0, 5; mid 2
    "tiny+mid": [400, 5, 300, 3, 7, 450],       # no table reaches B rows
    "big+mid": [600, 5, 300, 1000],             # a single table of <= 254 rows: the tiny form declines
    "tiny+big": [600, 5, 3, 7, 1000],           # no mid-size field: no row-sorted launch
}


def _mask(fields) -> str:
    return ",".join(str(f) for f in fields) or "-"


def _bits(skip: int) -> str:
    return _mask(f for f in range(64) if skip >> f & 1)


class Recorder:
    """stands in for the hip entry points and the LaunchPlan calls of the path; `log` is the issue order"""

    def __init__(self, monkeypatch, recording: bool, fail_in: str = None, smp_fits: bool = True):
        self.log, self.dw_ptrs, self.scopes, self.fail_in = [], set(), [], fail_in
        self.ss_marked, self.ss_made, self.ss_given = [], [], []
        for name in ("relu_bwd", "linear_wgrad", "linear_wgrad_xbf16", "transpose", "embed_grad_tiny", "embed_grad_smp",
                     "embed_grad_smp_mark", "embed_grad_ss_mark", "embed_grad_ss", "embed_grad_seg", "embed_grad_gemm"):
            monkeypatch.setattr(hip, name, getattr(self, name))
        monkeypatch.setattr(hip, "embed_grad_smp_fits", lambda D, hidden, dh: smp_fits)
        for name in ("fork2_mark", "side2_sync", "run_deferred", "join"):
            monkeypatch.setattr(hip.LaunchPlan, name, staticmethod(lambda name=name: self.log.append(name)))
        monkeypatch.setattr(hip.LaunchPlan, "section", staticmethod(lambda k: self.log.append(f"section({k})")))
        monkeypatch.setattr(hip.LaunchPlan, "is_recording", staticmethod(lambda: recording))
        monkeypatch.setattr(Fh, "_wgrad_stream", lambda device: None)

    def _launch(self, name, accumulate=None, dw="absent", **what):
        parts = [name] + [f"{k}={v}" for k, v in what.items()]
        if accumulate is not None:
            parts.append(f"acc={int(accumulate)}")
        parts.append(f"held={int(hip.holding.active())}")  # inside a hip.holding() block: what the launch allocates stays
        if hip.holding.active():
            self.scopes.append(hip._HOLDING)
        if dw != "absent":
            parts.append("dw=" + ("None" if dw is None else "shared"))
            if dw is not None:
                self.dw_ptrs.add(dw.data_ptr())
        self.log.append(" ".join(parts))
        if name == self.fail_in:
            raise RuntimeError(f"{name} fails")

    def relu_bwd(self, dy, act_out):
        self._launch("relu_bwd")
        return torch.zeros_like(dy)

    def transpose(self, w, rows_out=None):
        self._launch("transpose")
        return torch.zeros((rows_out or w.shape[1], w.shape[0]))

    def linear_wgrad(self, dy, x, K, dw=None, db=None, accumulate=False, want_bias=True):
        self._launch("linear_wgrad", cols=K, out="new" if dw is None else "view")
        return (dw if dw is not None else torch.zeros((dy.shape[1], K))), (torch.zeros(dy.shape[1]) if want_bias else None)

    def linear_wgrad_xbf16(self, dy, x16, K, want_bias=True):
        self._launch("linear_wgrad_xbf16", cols=K)
        return torch.zeros((dy.shape[1], K)), (torch.zeros(dy.shape[1]) if want_bias else None)

    def embed_grad_tiny(self, keys, B, tiny, dh, wt, gfm, sum_in, arena, grad_arena, accumulate, dw=None):
        self._launch("embed_grad_tiny", fields=_mask(t[0] for t in tiny), accumulate=accumulate, dw=dw)

    def embed_grad_smp_mark(self, sorted_keys, sorted_pos, B, fields, out=None):
        self._launch("embed_grad_smp_mark", fields=_mask(fields))
        return out if out is not None else tuple(torch.zeros(1, dtype=torch.int32) for _ in range(3))

    def embed_grad_smp(self, keys, marks, B, F, fields, dh, w, gfm, sum_in, arena, grad_arena, accumulate, dw=None, phases=3,
                       ws=None):
        assert marks is not None and (phases == 1 or ws == "smp workspace")
        self._launch(f"embed_grad_smp[{phases}]", fields=_mask(t[0] for t in fields), accumulate=accumulate, dw=dw)
        return "smp workspace" if phases == 1 else None

    def embed_grad_ss_mark(self, sorted_keys, B, skip_fields, out=None):
        self._launch("embed_grad_ss_mark", skip=_bits(skip_fields))
        self.ss_marked.append(skip_fields)
        self.ss_made.append(out if out is not None else tuple(torch.zeros(1, dtype=torch.int32) for _ in range(3)))
        return self.ss_made[-1]

    def embed_grad_ss(self, sorted_keys, sorted_pos, B, D, dh, w, gfm, sum_in, arena, grad_arena, accumulate,
                      skip_fields=0, field_rows=None, dw=None, phases=3, ws=None, marks=None):
        self.ss_given.append((skip_fields, marks))
        self._launch("embed_grad_ss", skip=_bits(skip_fields), marks="None" if marks is None else "sort",
                     accumulate=accumulate, dw=dw)

    def embed_grad_seg(self, sorted_keys, sorted_pos, B, D, dh, w, gfm, sum_in, arena, grad_arena, accumulate,
                       skip_fields=0, field_rows=None, dw=None):
        self._launch("embed_grad_seg", skip=_bits(skip_fields), accumulate=accumulate, dw=dw)

    def embed_grad_gemm(self, sorted_keys, sorted_pos, B, D, dh, wt, dx, gfm, sum_in, arena, grad_arena, accumulate,
                        skip_fields=0):
        assert dx is None
        self._launch("embed_grad_gemm", skip=_bits(skip_fields), accumulate=accumulate)


def _marks_in(log):
    return [entry for entry in log if entry.startswith(("embed_grad_smp_mark", "embed_grad_ss_mark"))]


def _layer(rows):
    layer = E.EmbeddingLayer({f"C{f}": {"vocab_size": r - 1} for f, r in enumerate(rows)}, 64)
    assert layer._rows_sig() == tuple(rows)
    return layer


def _lookup(layer, batch: int = B):
    """the field-major arena rows of a batch and their sort, as EmbeddingLayer._sorted_keys would hand them on"""
    g = torch.Generator().manual_seed(5)
    rows = layer._rows_sig()
    keys = torch.cat([sum(rows[:f]) + torch.randint(0, r, (batch,), generator=g) for f, r in enumerate(rows)]).to(torch.int32)
    sk, sp = torch.sort(keys, stable=True)
    return E.SortedLookup(keys, sk, sp.to(torch.int32))


def _backward(layer, look, x_mode: str, batch: int = B):
    """_EmbedGatherLinear.backward with a stand-in ctx (what its forward leaves behind); -> the weight gradient"""
    F = len(layer.emb_feature)
    K = F * 64 + ND
    ldx = (K + 63) // 64 * 64
    x = torch.zeros((batch, 64 if x_mode == "seg" else ldx), dtype=torch.bfloat16 if x_mode == "bf16" else torch.float32)
    ctx = SimpleNamespace(saved_tensors=(look.keys, None, x, torch.zeros((batch, 64)), torch.zeros((64, K))),
                          store=layer, out_link=None, needs_input_grad=[False] * 4 + [True, True, False, False] + [True] * F,
                          has_bias=True, x_mode=x_mode, K=K, Kg=F * 64, ldx=ldx, wt=None, need_tables=True, B=batch,
                          presorted=look)
    out = Fh._EmbedGatherLinear.backward(ctx, torch.zeros((batch, 64)), None)
    assert len(out) == 8 + F and out[5] is not None
    return out[4]


def _run(monkeypatch, tables: str, recording: bool, x_mode: str, premarked: bool = False, **rec_kw):
    rec = Recorder(monkeypatch, recording, **rec_kw)
    layer = _layer(TABLES[tables])
    look = _lookup(layer)
    if premarked:  # the marks made behind the sort, as for a sort started ahead
        layer._marks_wanted = True
        layer._mark_sorted(look)
        del rec.log[:]
    dw = _backward(layer, look, x_mode)
    assert rec.dw_ptrs <= {dw.data_ptr()}          # every `dw=shared` above is the buffer the node returns
    assert all(sc is rec.scopes[0] for sc in rec.scopes)  # every `held=1` launch of this backward saw the same scope list
    assert not hip.holding.active()
    return rec


# recorded on the parent of the change that gathered this backward into one function (see the module docstring)
EXPECTED = {
    ('tiny+big+mid', True, 'seg'): [
        'relu_bwd held=0',
        'transpose held=1',
        'fork2_mark',
        'embed_grad_smp_mark fields=0,5 held=1',
        'embed_grad_ss_mark skip=0,1,3,4,5 held=1',
        'embed_grad_smp[1] fields=0,5 acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=shared',
        'section(0)',
        'side2_sync',
        'embed_grad_ss skip=0,1,3,4,5 marks=sort acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_smp[2] fields=0,5 acc=0 held=1 dw=shared',
        'section(0)',
        'section(2)',
        'linear_wgrad cols=13 out=view held=1',
        'run_deferred',
        'section(0)',
        'join',
    ],
    ('tiny+big+mid', True, 'full'): [
        'relu_bwd held=0',
        'section(2)',
        'linear_wgrad cols=397 out=new held=1',
        'run_deferred',
        'section(0)',
        'transpose held=1',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=None',
        'section(0)',
        'embed_grad_gemm skip=1,3,4 acc=0 held=1',
        'join',
    ],
    ('tiny+big+mid', False, 'seg'): [
        'relu_bwd held=0',
        'linear_wgrad cols=13 out=view held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=shared',
        'embed_grad_smp_mark fields=0,5 held=0',
        'embed_grad_ss_mark skip=0,1,3,4,5 held=0',
        'embed_grad_smp[1] fields=0,5 acc=0 held=0 dw=shared',
        'embed_grad_ss skip=0,1,3,4,5 marks=sort acc=0 held=0 dw=shared',
        'embed_grad_smp[2] fields=0,5 acc=0 held=0 dw=shared',
    ],
    ('tiny+big+mid', False, 'full'): [
        'relu_bwd held=0',
        'linear_wgrad cols=397 out=new held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=None',
        'embed_grad_gemm skip=1,3,4 acc=0 held=0',
    ],
    ('tiny+mid', True, 'seg'): [
        'relu_bwd held=0',
        'transpose held=1',
        'fork2_mark',
        'embed_grad_seg skip=1,3,4 acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=shared',
        'section(0)',
        'section(2)',
        'linear_wgrad cols=13 out=view held=1',
        'run_deferred',
        'section(0)',
        'join',
    ],
    ('tiny+mid', True, 'full'): [
        'relu_bwd held=0',
        'section(2)',
        'linear_wgrad cols=397 out=new held=1',
        'run_deferred',
        'section(0)',
        'transpose held=1',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=None',
        'section(0)',
        'embed_grad_gemm skip=1,3,4 acc=0 held=1',
        'join',
    ],
    ('tiny+mid', False, 'seg'): [
        'relu_bwd held=0',
        'linear_wgrad cols=13 out=view held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=shared',
        'embed_grad_seg skip=1,3,4 acc=0 held=0 dw=shared',
    ],
    ('tiny+mid', False, 'full'): [
        'relu_bwd held=0',
        'linear_wgrad cols=397 out=new held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=None',
        'embed_grad_gemm skip=1,3,4 acc=0 held=0',
    ],
    ('big+mid', True, 'seg'): [
        'relu_bwd held=0',
        'transpose held=1',
        'embed_grad_smp_mark fields=0,3 held=1',
        'embed_grad_ss_mark skip=0,3 held=1',
        'embed_grad_smp[1] fields=0,3 acc=0 held=1 dw=shared',
        'fork2_mark',
        'embed_grad_ss skip=0,3 marks=sort acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_smp[2] fields=0,3 acc=0 held=1 dw=shared',
        'section(0)',
        'section(2)',
        'linear_wgrad cols=13 out=view held=1',
        'run_deferred',
        'section(0)',
        'join',
    ],
    ('big+mid', True, 'full'): [
        'relu_bwd held=0',
        'section(2)',
        'linear_wgrad cols=269 out=new held=1',
        'run_deferred',
        'section(0)',
        'transpose held=1',
        'embed_grad_gemm skip=- acc=0 held=1',
        'join',
    ],
    ('big+mid', False, 'seg'): [
        'relu_bwd held=0',
        'linear_wgrad cols=13 out=view held=0',
        'transpose held=0',
        'embed_grad_smp_mark fields=0,3 held=0',
        'embed_grad_ss_mark skip=0,3 held=0',
        'embed_grad_smp[1] fields=0,3 acc=0 held=0 dw=shared',
        'embed_grad_ss skip=0,3 marks=sort acc=0 held=0 dw=shared',
        'embed_grad_smp[2] fields=0,3 acc=0 held=0 dw=shared',
    ],
    ('big+mid', False, 'full'): [
        'relu_bwd held=0',
        'linear_wgrad cols=269 out=new held=0',
        'transpose held=0',
        'embed_grad_gemm skip=- acc=0 held=0',
    ],
    ('tiny+big', True, 'seg'): [
        'relu_bwd held=0',
        'transpose held=1',
        'fork2_mark',
        'embed_grad_smp_mark fields=0,4 held=1',
        'embed_grad_smp[1] fields=0,4 acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_tiny fields=1,2,3 acc=0 held=1 dw=shared',
        'section(0)',
        'side2_sync',
        'section(2)',
        'embed_grad_smp[2] fields=0,4 acc=0 held=1 dw=shared',
        'section(0)',
        'section(2)',
        'linear_wgrad cols=13 out=view held=1',
        'run_deferred',
        'section(0)',
        'join',
    ],
    ('tiny+big', True, 'full'): [
        'relu_bwd held=0',
        'section(2)',
        'linear_wgrad cols=333 out=new held=1',
        'run_deferred',
        'section(0)',
        'transpose held=1',
        'section(2)',
        'embed_grad_tiny fields=1,2,3 acc=0 held=1 dw=None',
        'section(0)',
        'embed_grad_gemm skip=1,2,3 acc=0 held=1',
        'join',
    ],
    ('tiny+big', False, 'seg'): [
        'relu_bwd held=0',
        'linear_wgrad cols=13 out=view held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,2,3 acc=0 held=0 dw=shared',
        'embed_grad_smp_mark fields=0,4 held=0',
        'embed_grad_smp[1] fields=0,4 acc=0 held=0 dw=shared',
        'embed_grad_smp[2] fields=0,4 acc=0 held=0 dw=shared',
    ],
    ('tiny+big', False, 'full'): [
        'relu_bwd held=0',
        'linear_wgrad cols=333 out=new held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,2,3 acc=0 held=0 dw=None',
        'embed_grad_gemm skip=1,2,3 acc=0 held=0',
    ],
    ('tiny+big+mid', True, 'seg', 'RP_SS_MARK_AHEAD=0'): [
        'relu_bwd held=0',
        'transpose held=1',
        'fork2_mark',
        'embed_grad_smp_mark fields=0,5 held=1',
        'embed_grad_smp[1] fields=0,5 acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=shared',
        'section(0)',
        'side2_sync',
        'embed_grad_ss skip=0,1,3,4,5 marks=None acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_smp[2] fields=0,5 acc=0 held=1 dw=shared',
        'section(0)',
        'section(2)',
        'linear_wgrad cols=13 out=view held=1',
        'run_deferred',
        'section(0)',
        'join',
    ],
    ('tiny+big+mid', True, 'seg', 'premarked'): [
        'relu_bwd held=0',
        'transpose held=1',
        'fork2_mark',
        'embed_grad_smp[1] fields=0,5 acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=shared',
        'section(0)',
        'side2_sync',
        'embed_grad_ss skip=0,1,3,4,5 marks=sort acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_smp[2] fields=0,5 acc=0 held=1 dw=shared',
        'section(0)',
        'section(2)',
        'linear_wgrad cols=13 out=view held=1',
        'run_deferred',
        'section(0)',
        'join',
    ],
    ('tiny+big+mid', True, 'bf16'): [
        'relu_bwd held=0',
        'section(2)',
        'linear_wgrad_xbf16 cols=397 held=1',
        'run_deferred',
        'section(0)',
        'transpose held=1',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=None',
        'section(0)',
        'embed_grad_gemm skip=1,3,4 acc=0 held=1',
        'join',
    ],
    ('tiny+big+mid', True, 'seg', 'smp does not fit'): [
        'relu_bwd held=0',
        'transpose held=1',
        'fork2_mark',
        'embed_grad_seg skip=1,3,4 acc=0 held=1 dw=shared',
        'section(2)',
        'embed_grad_tiny fields=1,3,4 acc=0 held=1 dw=shared',
        'section(0)',
        'section(2)',
        'linear_wgrad cols=13 out=view held=1',
        'run_deferred',
        'section(0)',
        'join',
    ],
    ('tiny+big+mid', False, 'seg', 'RP_SS_MARK_AHEAD=0'): [
        'relu_bwd held=0',
        'linear_wgrad cols=13 out=view held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=shared',
        'embed_grad_smp_mark fields=0,5 held=0',
        'embed_grad_smp[1] fields=0,5 acc=0 held=0 dw=shared',
        'embed_grad_ss skip=0,1,3,4,5 marks=None acc=0 held=0 dw=shared',
        'embed_grad_smp[2] fields=0,5 acc=0 held=0 dw=shared',
    ],
    ('tiny+big+mid', False, 'seg', 'premarked'): [
        'relu_bwd held=0',
        'linear_wgrad cols=13 out=view held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=shared',
        'embed_grad_smp[1] fields=0,5 acc=0 held=0 dw=shared',
        'embed_grad_ss skip=0,1,3,4,5 marks=sort acc=0 held=0 dw=shared',
        'embed_grad_smp[2] fields=0,5 acc=0 held=0 dw=shared',
    ],
    ('tiny+big+mid', False, 'bf16'): [
        'relu_bwd held=0',
        'linear_wgrad_xbf16 cols=397 held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=None',
        'embed_grad_gemm skip=1,3,4 acc=0 held=0',
    ],
    ('tiny+big+mid', False, 'seg', 'smp does not fit'): [
        'relu_bwd held=0',
        'linear_wgrad cols=13 out=view held=0',
        'transpose held=0',
        'embed_grad_tiny fields=1,3,4 acc=0 held=0 dw=shared',
        'embed_grad_seg skip=1,3,4 acc=0 held=0 dw=shared',
    ],
}


CASES = [(t, r, m) for t in TABLES for r in (True, False) for m in ("seg", "full")]


@pytest.mark.parametrize("tables,recording,x_mode", CASES)
def test_issue_order(monkeypatch, tables, recording, x_mode):
    rec = _run(monkeypatch, tables, recording, x_mode)
    assert rec.log == EXPECTED[tables, recording, x_mode]


@pytest.mark.parametrize("recording", [True, False])
def test_issue_order_without_lists_made_with_the_sort(monkeypatch, recording):
    """RP_SS_MARK_AHEAD=0: no unique-row lists behind the sort, rp_embed_grad_ss makes its own"""
    monkeypatch.setenv("RP_SS_MARK_AHEAD", "0")
    rec = _run(monkeypatch, "tiny+big+mid", recording, "seg")
    assert rec.log == EXPECTED["tiny+big+mid", recording, "seg", "RP_SS_MARK_AHEAD=0"]
    assert not rec.ss_marked and rec.ss_given == [(0b111011, None)]


@pytest.mark.parametrize("recording", [True, False])
def test_issue_order_with_a_sort_that_carries_its_marks(monkeypatch, recording):
    rec = _run(monkeypatch, "tiny+big+mid", recording, "seg", premarked=True)
    assert not _marks_in(rec.log)
    assert rec.log == EXPECTED["tiny+big+mid", recording, "seg", "premarked"]


@pytest.mark.parametrize("recording", [True, False])
def test_issue_order_bf16_activation(monkeypatch, recording):
    """bf16-storage training with RP_GRAD_SEG=0: the stored bf16 activation's weight gradient, then as `full`"""
    rec = _run(monkeypatch, "tiny+big+mid", recording, "bf16")
    assert rec.log == EXPECTED["tiny+big+mid", recording, "bf16"]


@pytest.mark.parametrize("recording", [True, False])
def test_issue_order_when_the_sample_major_form_does_not_fit(monkeypatch, recording):
    rec = _run(monkeypatch, "tiny+big+mid", recording, "seg", smp_fits=False)
    assert rec.log == EXPECTED["tiny+big+mid", recording, "seg", "smp does not fit"]


@pytest.mark.parametrize("tables,x_mode,fail_in", [("tiny+big+mid", "seg", "embed_grad_tiny"),
                                                   ("tiny+big+mid", "seg", "embed_grad_smp[2]"),
                                                   ("tiny+big+mid", "seg", "linear_wgrad"),
                                                   ("tiny+mid", "seg", "embed_grad_tiny"),
                                                   ("tiny+big+mid", "full", "embed_grad_tiny"),
                                                   ("tiny+big+mid", "full", "linear_wgrad")])
def test_a_failing_side_launch_still_returns_to_the_main_section(monkeypatch, tables, x_mode, fail_in):
    rec = Recorder(monkeypatch, True, fail_in=fail_in)
    layer = _layer(TABLES[tables])
    with pytest.raises(RuntimeError, match="fails"):
        _backward(layer, _lookup(layer), x_mode)
    assert rec.log[-2].startswith(fail_in) and rec.log[-1] == "section(0)"
    assert not hip.holding.active()  # the backward's holding() block is closed behind the exception
    assert rec.log.count("section(2)") == rec.log.count("section(0)")


@pytest.mark.parametrize("tables", list(TABLES))
@pytest.mark.parametrize("batch,min_batch", [(512, 512), (512, 513), (128, 128), (128, 129)])
@pytest.mark.parametrize("mark_ahead", [True, False])
def test_marks_made_with_the_sort_are_the_ones_the_backward_uses(monkeypatch, tables, batch, min_batch, mark_ahead):
    """the classification behind the sort (EmbeddingLayer._mark_sorted, possibly a step ahead on a side stream) and the
    one in the backward agree: the streaming form runs over exactly the fields whose unique-row lists were made, and is
    handed those lists"""
    monkeypatch.setenv("RP_SMP_MIN_BATCH", str(min_batch))
    if not mark_ahead:
        monkeypatch.setenv("RP_SS_MARK_AHEAD", "0")
    rec = Recorder(monkeypatch, recording=True)
    layer = _layer(TABLES[tables])
    look = _lookup(layer, batch)
    layer._marks_wanted = True  # (what the first three-form backward sets)
    layer._mark_sorted(look)
    marked, made = list(rec.ss_marked), list(rec.ss_made)
    n_marks = len(rec.log)
    _backward(layer, look, "seg", batch)
    assert not _marks_in(rec.log[n_marks:])  # the backward made none of its own
    ss = [entry for entry in rec.log if entry.startswith("embed_grad_ss ")]
    smp = [entry for entry in rec.log if entry.startswith("embed_grad_smp[1]")]
    rest = [entry for entry in rec.log if entry.startswith(("embed_grad_ss ", "embed_grad_seg "))]
    # the streaming form runs exactly when there are big tables (batch at or above the minimum) and mid-size fields
    rows = TABLES[tables]
    tiny = [f for f, r in enumerate(rows) if r <= 254]
    tiny = tiny if len(tiny) >= 2 else []
    big = [f for f, r in enumerate(rows) if f not in tiny and r >= batch and batch >= min_batch]
    mid = [f for f in range(len(rows)) if f not in tiny + big]
    assert bool(smp) == bool(big) and bool(ss) == bool(big and mid) and bool(rest) == bool(mid)
    if ss and mark_ahead:
        (skip, lists), = rec.ss_given
        assert marked == [skip] and lists is made[0] and look.ss_lists(skip) is made[0]
    else:
        assert not marked and all(lists is None for _, lists in rec.ss_given)
