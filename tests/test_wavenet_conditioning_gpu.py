"""-m gpu: generation at the conditioning geometries of tests/conditioning_cases.py -- local-condition widths 4 .. 128, one to four
upsampling stages (a factor of 1 among them), global-condition widths 1 .. 64 and the embedding passed in -- on every generation
kernel, BIT FOR BIT against the CPU oracle (helpers.first_mismatch: equality, no tolerance anywhere in this file).

Every test first asserts m.kernel_name() and m.fused_conditioning(): a case cannot pass on another kernel than the one it names.
The inputs are the sensitive ones (tests/sensitive_inputs.py, conditions asserted on the oracle's output by helpers.sensitive_mol /
sensitive_onehot); tests/test_wavenet_conditioning_cpu.py shows that they see the last channel and the last tap of every row.  A case
(model weights, mel frames, uniforms, the oracle's samples) is built once per process and shared by the tests that use it.

What the rows reach in the kernels:
  * lc_role / lc_many_role (XCD kernels): layers per lc wave 4 (l4, l20, l32f1), 2 (l36, l64), 1 (l68 .. l128) up to 30 layers and
    4 / 3 / 2 / 1 above; a ragged last wave at each; NLC 1 .. 4 with full and 4-wide last chunks; the wave-private rows of 128 floats
    full (l128); phase counters of one to four digits, a digit that never moves (l32f1);
  * lc_many_role's general chunk loop (every row but l68 / l96 / the G rows) and its paired fast path at its two edges (l68, l96 at
    ten streams on an XCD), the fall-through from its guard at NLC = 4 (l100 at ten streams);
  * the refusal of the many-streams kernel (l128): `xcd_many` = 1 ignored, batch 33 on the generic kernel;
  * wn_lc_kernel / wn_gc_kernel / wn_wide_proj_kernel with partial chunks, gc widths that are no multiple of 4, a second gc chunk."""
import numpy as np
import pytest

import conditioning_cases as CC
from helpers import first_mismatch

pytestmark = pytest.mark.gpu

XCD, MANY, GENERIC, WIDE = "wn_xcd_generate_kernel", "wn_xcd_many_kernel", "wn_generate_kernel", "wn_wide_generate_kernel"
EVERY_ROW = list(CC.ROWS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _routed(m, kernel, fused):
    assert m.kernel_name() == kernel, m.kernel_name()
    assert m.fused_conditioning() == fused
    return m


def _lazy(m, c):
    """the handle of create_upsample under fused conditioning: generate() upsamples the mel frames inside its launch (XLC_MEL)"""
    from twvk_amd.wavenet import Upsampled
    up = m.create_upsample(c.mel)
    assert isinstance(up, Upsampled) and up.shape == (c.B, c.mel.shape[1] * CC.hop(c.rid), c.kw["L"])
    return up


def _rows(m, c):
    """the rows of the stand-alone upsampling kernel, handed over as a tensor (XLC_UPSAMPLED on the XCD kernels)"""
    rows = m.create_upsample(c.mel, materialize=True)[:, :c.T].contiguous()
    assert first_mismatch(rows.cpu().numpy(), c.U) is None, ("upsample", c.rid, first_mismatch(rows.cpu().numpy(), c.U))
    return rows


def _same(got, c, what):
    got = got.cpu().numpy()
    assert got.shape == c.want.shape and got.dtype == c.want.dtype, (what, got.shape, got.dtype)
    assert first_mismatch(got, c.want) is None, (c.rid, what, "first mismatch (stream, step)", first_mismatch(got, c.want))
    return got


def _check_dumps(O, c, dump):
    """z, x of every layer and the raw outputs of the first DUMP_STEPS steps against the oracle's own (no sampler in between)"""
    dump = dump.cpu().numpy()
    NL, B = c.d.n_layers, c.B
    st = O.State(c.d, B)
    inp = c.first.copy()
    for t in range(CC.DUMP_STEPS):
        raw, dz, dx = O.step(c.d, c.blob, st, inp, c.U[:, t], c.gc, debug=True)
        gz = dump[:, t, :NL * 64].reshape(B, NL, 2, 32)
        assert first_mismatch(gz[:, :, 0], dz) is None, (c.rid, "z: step, (stream, layer, channel)", t, first_mismatch(gz[:, :, 0], dz))
        assert first_mismatch(gz[:, :, 1], dx) is None, (c.rid, "x: step, (stream, layer, channel)", t, first_mismatch(gz[:, :, 1], dx))
        graw = dump[:, t, NL * 64:NL * 64 + c.d.O]
        assert first_mismatch(graw, raw) is None, (c.rid, "raw", t, first_mismatch(graw, raw))
        inp = c.want[:, t]


def _report(c, m, what):
    clamp, edges = c.figures()
    print("parity %-7s %-26s %-22s fused %d layers %2d B %2d T %3d clamp %s edges %.3f" % (
        c.rid, what, m.kernel_name(), m.fused_conditioning(), c.d.n_layers, c.B, c.T, "  -  " if clamp is None else "%.3f" % clamp, edges))


# ---------------------------------------------------------------------------------------------------------------- create_upsample alone
@pytest.mark.parametrize("rid", CC.L_ROWS)
def test_create_upsample(torch_cuda, oracle, rid):
    """wn_upsample_stage_kernel at every width and upsampling list, (B, T_mel) = (2, 3) and (1, 1)"""
    c = CC.case(oracle, rid, 3)
    m = CC.model(c, B=2)
    rng = np.random.RandomState(len(rid))
    for B, Tm in ((2, 3), (1, 1)):
        mel = rng.uniform(-4, 4, (B, Tm, c.kw["L"])).astype(np.float32)
        got = m.create_upsample(mel, materialize=True).cpu().numpy()
        want = oracle.upsample(c.d, c.blob, mel)
        assert got.shape == want.shape == (B, Tm * CC.hop(rid), c.kw["L"])
        assert first_mismatch(got, want) is None, (rid, B, Tm, first_mismatch(got, want))


# ---------------------------------------------------------------------------------------------------------------- generic kernel
@pytest.mark.parametrize("rid", EVERY_ROW)
def test_generic_kernel(torch_cuda, oracle, rid):
    """wn_lc_kernel / wn_gc_kernel and the generic kernel: the dumps of the first 16 steps (at the small hops: several frame
    boundaries), then the samples"""
    c = CC.case(oracle, rid, 3)
    m = _routed(CC.model(c, xcd=0), GENERIC, False)
    got, dump = m.generate(_rows(m, c), c.gc, c.first, c.u, debug_steps=CC.DUMP_STEPS)
    _check_dumps(oracle, c, dump)
    _same(got, c, "generic")
    m.queue_initializer()
    _same(m.generate(_rows(m, c), c.gc, c.first, c.u), c, "generic, no dumps")
    _report(c, m, "generic")


# ---------------------------------------------------------------------------------------------------------------- XCD kernel
def _xcd_both_ways(oracle, c, dumps):
    """the lazy handle (fused: XLC_MEL) and the materialised rows (XLC_UPSAMPLED) on wn_xcd_generate_kernel, against the oracle and so
    against each other; with dumps, each once more on the instrumented build of the 30-layer kernel"""
    m = _routed(CC.model(c), XCD, True)
    a = _same(m.generate(_lazy(m, c), c.gc, c.first, c.u), c, "xcd, mel frames")
    m.queue_initializer()
    b = _same(m.generate(_rows(m, c), c.gc, c.first, c.u), c, "xcd, upsampled rows")
    assert first_mismatch(a, b) is None
    for what, src in (("xcd, mel frames, dumps", _lazy), ("xcd, upsampled rows, dumps", _rows)) if dumps else ():
        m.queue_initializer()
        got, dump = m.generate(src(m, c), c.gc, c.first, c.u, debug_steps=CC.DUMP_STEPS)
        _check_dumps(oracle, c, dump)
        _same(got, c, what)
    _report(c, m, "xcd mel+rows")


@pytest.mark.parametrize("rid,nl", [(r, 7) for r in EVERY_ROW] + [("l4", 30), ("l64", 30), ("l100", 30), ("l4", 9)])
def test_xcd_kernel(torch_cuda, oracle, rid, nl):
    """7 layers: every row.  30 layers: 4 / 2 / 1 layers per lc wave with full waves (8 / 15 / 30 waves: one, two and four lc
    workgroups); l4 at 9 layers: the last wave owns one layer of four"""
    _xcd_both_ways(oracle, CC.case(oracle, rid, 3, n_layers=nl), dumps=True)


@pytest.mark.parametrize("rid,nl", [("l4", 31), ("l64", 33), ("l80", 31), ("l100", 41)])
def test_xcd_kernel_above_30_layers(torch_cuda, oracle, rid, nl):
    """two chain workgroups, six register tiles per lc wave: l4 at 31 layers gives a wave four layers and the last wave three, l64 at
    33 three (six tiles), the default geometry at 31 two with a last wave of one, l100 at 41 one.  (No instrumented build here.)"""
    _xcd_both_ways(oracle, CC.case(oracle, rid, 2, n_layers=nl), dumps=False)


@pytest.mark.parametrize("rid", ["l20", "g33"])
def test_xcd_kernel_onehot(torch_cuda, oracle, rid):
    """the one-hot mu-law-256 model's instantiation of the XCD kernel: class ids equal to the checker's"""
    c = CC.case(oracle, rid, 2, scalar=False)
    assert c.want.dtype == np.int32
    _xcd_both_ways(oracle, c, dumps=True)


# ---------------------------------------------------------------------------------------------------------------- many-streams kernel
@pytest.mark.parametrize("rid", [r for r in EVERY_ROW if r != "l128"])
def test_many_streams_kernel(torch_cuda, oracle, rid):
    """`xcd_many` = 1 at B = 9: XCD 0 carries two streams, both slots of a chain workgroup; mel frames and upsampled rows"""
    c = CC.case(oracle, rid, 9)
    m = _routed(CC.model(c, xcd_many=1), MANY, True)
    _same(m.generate(_lazy(m, c), c.gc, c.first, c.u), c, "many, mel frames")
    m.queue_initializer()
    _same(m.generate(_rows(m, c), c.gc, c.first, c.u), c, "many, upsampled rows")
    _report(c, m, "many mel+rows")


@pytest.mark.parametrize("rid", ["l68", "l96", "l100"])
def test_many_streams_kernel_ten_streams_on_an_xcd(torch_cuda, oracle, rid):
    """B = 75: XCDs 0 .. 2 hold ten streams, the others nine.  l68 and l96 take lc_many_role's paired fast path (ns > 9, NLC = 3,
    Lc <= 96) on the rows that only move the last stage and the general body on the others; l100 (NLC = 4) falls through the guard"""
    c = CC.case(oracle, rid, 75)
    m = _routed(CC.model(c), MANY, True)
    _same(m.generate(_lazy(m, c), c.gc, c.first, c.u), c, "many, 75 streams")
    _report(c, m, "many mel")


def test_many_streams_kernel_refused_at_l128(torch_cuda, oracle):
    """(n_up + 1) * NLC = 20 rows per stream do not fit an lc wave's eighth of the LDS: `xcd_many` = 1 is ignored (the batch <= 32 kernel
    runs, same samples), and a batch above 32 goes to the generic kernel"""
    c = CC.case(oracle, "l128", 9)
    m = _routed(CC.model(c, xcd_many=1), XCD, True)
    _same(m.generate(_lazy(m, c), c.gc, c.first, c.u), c, "xcd at xcd_many = 1")
    _report(c, m, "xcd_many=1 ignored")
    c = CC.case(oracle, "l128", 33)
    m = _routed(CC.model(c), GENERIC, False)
    _same(m.generate(_rows(m, c), c.gc, c.first, c.u), c, "generic at batch 33")
    _report(c, m, "batch 33")


# ---------------------------------------------------------------------------------------------------------------- wide kernel
@pytest.mark.parametrize("rid", ["l20", "l100", "g5", "g33", "g48emb"])
def test_wide_kernel(torch_cuda, oracle, rid):
    """wn_wide_proj_kernel (zero-padded partial chunks) in front of wn_wide_generate_kernel at R = D = 64"""
    import test_wavenet_wide_gpu as wide
    c = CC.case(oracle, rid, 2, builder=lambda O, dil, **kw: wide.make_case(O, dil, 64, 64, scale=CC.SCALE, **kw), tag="wide64")
    assert (c.d.R, c.d.D) == (64, 64)
    m = _routed(wide.make_model(2, c.dil, c.tensors, 64, 64, **c.kw), WIDE, False)
    _same(m.generate(_rows(m, c), c.gc, c.first, c.u), c, "wide")
    _report(c, m, "wide 64x64")


# ---------------------------------------------------------------------------------------------------------------- calls in pieces
@pytest.mark.parametrize("rid,B,kernel", [("l64", 3, XCD), ("l100", 3, XCD), ("l64", 9, MANY), ("l100", 9, MANY)])
def test_calls_in_pieces(torch_cuda, oracle, rid, B, kernel):
    """the same T as calls of 1, 5, 17 and the rest, the state carried over (delay lines, causal queue, the last lc frame in st_lcprev):
    launches of at most ring + 1 steps wait for the previous launch's frame to be consumed before they overwrite its slot"""
    c = CC.case(oracle, rid, B)
    m = _routed(CC.model(c, **(dict(xcd_many=1) if kernel == MANY else {})), kernel, True)
    U = _rows(m, c)
    outs, fi, p = [], c.first, 0
    for n in (1, 5, 17, c.T - 23):
        o = m.generate(U[:, p:p + n].contiguous(), c.gc, fi, c.u[:, p:p + n]).cpu().numpy()
        outs.append(o); fi = o[:, -1]; p += n
    assert p == c.T
    got = np.concatenate(outs, axis=1)
    assert first_mismatch(got, c.want) is None, (rid, kernel, first_mismatch(got, c.want))
    _report(c, m, "calls of 1, 5, 17, rest")


# ---------------------------------------------------------------------------------------------------------------- priming
@pytest.mark.parametrize("B,kernel", [(3, XCD), (9, MANY)])
def test_priming_then_generation(torch_cuda, oracle, B, kernel):
    """generate.py:168-180 at l20: RF - 1 teacher-forced samples with zero local conditioning (rows of 20 zeros handed over), then
    generation from mel frames"""
    c = CC.case(oracle, "l20", B, primed=True)
    m = _routed(CC.model(c, **(dict(xcd_many=1) if kernel == MANY else {})), kernel, True)
    assert c.prime.shape[1] == oracle.receptive_field(c.d) == m.receptive_field
    m.prime(c.prime[:, :-1], None, c.gc)
    _same(m.generate(_lazy(m, c), c.gc, c.prime[:, -1], c.u), c, "primed")
    _report(c, m, "primed")
