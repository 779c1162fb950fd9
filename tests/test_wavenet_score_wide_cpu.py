"""Host-only side of the wide WaveNet scoring tests (residual_channels = dilation_channels = 64 and 128): route, workspace and views of
every table case of tests/score_wide_cases.py, the width refusals of both create functions, the fused route's size rule at its
boundary, the twv_wavenet_score_view export, this file's checker against torch_train_ref.network, and the window decomposition in
the float64 checker at the wide widths."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import score_wide_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 2


# ---- route, workspace, views ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", WC.IDS)
def test_case_is_on_the_route_it_is_meant_to_cover(cid):
    c = WC.case(cid)
    assert c.route["width"] == str(c.W) and c.W in (64, 128)
    for wf in c.windows:
        route, ws, views = WC.host_route(c, wf)
        assert {k: route[k] for k in c.route} == c.route, (cid, route)
        assert ws == 4 * int(route["carve_floats"])
        ow = wf * c.hop - c.rf
        O = c.kw.get("out_channels", 30) if c.kw.get("scalar_input", True) else c.kw.get("Q", 256)
        assert views["zc"][1:] == (c.slots * ow, c.n_layers * c.W) and views["y"][1:] == (c.slots * ow, O)
        for off, rows, cols in views.values():                       # both arrays lie inside the workspace, and apart
            assert 0 <= off and 4 * (off + rows * cols) <= ws
        (oz, rz, kz), (oy, _, _) = views["zc"], views["y"]
        assert oz + rz * kz <= oy


def test_width_32_twin_keeps_its_route_and_gains_the_width_key():
    route, ws, views = WC.host_route(WC.case("w64-small", 32))
    assert route["width"] == "32" and route["lc"] == "fused" and ws == 4 * int(route["carve_floats"])
    assert views["zc"][2] == 5 * 32


def test_workspace_grows_with_the_width():
    ws = [WC.host_route(WC.case("w64-small", W))[1] for W in (32, 64, 128)]
    assert ws[2] > ws[1] > ws[0], ws


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
class _Edited(object):
    """the dims edited behind the Python model (which has refusals of its own)"""

    def __init__(self, net, **over):
        from twvk_amd import _lib
        self._dims = _lib.Dims.from_buffer_copy(net._dims)
        for k, v in over.items():
            setattr(self._dims, k, v)


def test_unequal_and_other_widths_are_refused():
    from twvk_amd import _lib
    net = WC.case("w64-small").model("cpu")
    for R, D in ((64, 32), (32, 64), (128, 64), (96, 96), (16, 16), (256, 256)):
        rc, _, L = WC.create(_Edited(net, residual_channels=R, dilation_channels=D)._dims, 2, 900)
        assert rc == UNSUPPORTED, (R, D, rc)
        assert b"32, 64 or 128" in L.twv_last_error(), (R, D)
    for W in (32, 64, 128):
        rc, h, L = WC.create(_Edited(net, residual_channels=W, dilation_channels=W)._dims, 2, 900)
        assert rc == 0, W
        assert ("width=%d" % W).encode() in L.twv_wavenet_score_route(h)
        L.twv_wavenet_score_destroy(h)
    # the training step stays at 32, with the text it had
    L = _lib.lib()
    h = C.c_void_p()
    for R, D in ((64, 64), (128, 128), (64, 32)):
        assert L.twv_wavenet_train_create(C.byref(_Edited(net, residual_channels=R, dilation_channels=D)._dims), 2, 900, C.byref(h)) == UNSUPPORTED
        assert b"training is built for residual_channels = dilation_channels = 32 only: training at other widths is not built" in L.twv_last_error()


@pytest.mark.parametrize("W", [64, 128])
def test_fused_route_size_rule_is_the_same_at_every_width(W):
    """slots x window x 256 >= 2^31 is refused on the fused lc route whatever the width (the wide layer kernel addresses with 64 bits, so
    the bound does not shrink with W); the staged route takes it"""
    net = WC.case("w64-small", W).model("cpu")
    assert WC.create(net._dims, 64, 131100)[0] == UNSUPPORTED         # 64 * 131100 * 256 = 2^31 + 1.0 M
    rc, h, L = WC.create(net._dims, 64, 130800)                       # 2^31 - 4.3 M
    assert rc == 0
    assert L.twv_wavenet_score_workspace_bytes(h) > 64 * 130800 * W * 4 * 2
    L.twv_wavenet_score_destroy(h)
    rc, h, L = WC.create(WC.case("w64-staged", W).model("cpu")._dims, 64, 131072)
    assert rc == 0 and b"lc=staged" in L.twv_wavenet_score_route(h)
    L.twv_wavenet_score_destroy(h)


# ---- the view export ---------------------------------------------------------------------------------------------------------------
def test_view_export():
    from twvk_amd import _lib
    name = "twv_wavenet_score_view"
    header = open(os.path.join(ROOT, "include", "twv_amd.h")).read()
    L = _lib.lib()
    assert re.search(r"\b%s\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name)
    rc, h, _ = WC.create(WC.case("w128-small").model("cpu")._dims, 2, 900)
    assert rc == 0
    o, r, k = C.c_longlong(), C.c_longlong(), C.c_longlong()
    try:
        assert L.twv_wavenet_score_view(h, b"x", C.byref(o), C.byref(r), C.byref(k)) == INVALID
        assert b"unknown" in L.twv_last_error()
        assert L.twv_wavenet_score_view(h, b"zc", None, C.byref(r), C.byref(k)) == INVALID
        assert L.twv_wavenet_score_view(None, b"zc", C.byref(o), C.byref(r), C.byref(k)) == INVALID
        assert L.twv_wavenet_score_view(h, b"zc", C.byref(o), C.byref(r), C.byref(k)) == 0
        assert (r.value, k.value) == (2 * (900 - 42), 5 * 128) and o.value % 64 == 0
    finally:
        L.twv_wavenet_score_destroy(h)
    from twvk_amd.score import WaveNetScorer
    sc = WaveNetScorer(WC.case("w128-small").model("cpu"), window=900, slots=2)
    with pytest.raises(RuntimeError):
        sc.view("zc")                                                 # nothing has run: there is no workspace to look into


# ---- the checker --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["w64-small", "w128-small", "w64-onehot-q256"])
def test_matmul_form_checker_gives_the_conv_form_s_output(cid):
    """network_mm_z's y against torch_train_ref.network on one utterance in float64: 1e-12 of max|y| (measured 2.8e-17 and 1.1e-16
    absolute at 64 and 128); it returns one (len - rf, W) block of z per layer"""
    import torch_train_ref as R
    c = WC.case(cid)
    q = None if c.quantized is None else c.quantized[1]
    y, zs = WC.ref_views(c, c.audios[1], c.mels[1], c.gcs[1], q)
    want, _ = WC.ref_views(c, c.audios[1], c.mels[1], c.gcs[1], q, net=R.network)
    e = float(np.abs(y - want).max()) / float(np.abs(want).max())
    print("%s: matmul form against conv form, %.3g of max|y|" % (cid, e))
    assert y.shape == want.shape and e <= 1e-12
    assert len(zs) == c.n_layers and all(z.shape == (c.lengths[1] - c.rf, c.W) for z in zs)
    assert min(float(np.abs(z).max(axis=0).min()) for z in zs) > 0.0  # every channel of every layer says something


@pytest.mark.parametrize("cid", ["w64-small", "w128-one-cycle"])
def test_windows_through_the_checker_give_the_whole_utterance(cid):
    """the property of test_wavenet_score_cpu.py at the wide widths, with its tolerance: 1e-12 of max|nll64|"""
    from twvk_amd import score as S
    import score_cases as SC
    c = WC.case(cid)
    n64, n32 = WC.reference(cid)
    worst = 0.0
    for wf in c.windows:
        p = S.plan(c.lengths, wf * c.hop, c.rf, c.hop, c.slots)
        got = [np.full(T - c.rf, np.nan) for T in c.lengths]
        for u, start, n, first, last in p.table.reshape(-1, 5):
            if u < 0:
                continue
            v = SC.ref_nll(c, c.audios[u][start:start + n], c.mels[u][start // c.hop:(start + n) // c.hop], c.gcs[u], None)
            got[u][first - c.rf:last + 1 - c.rf] = v[first - start - c.rf:last + 1 - start - c.rf]
        for g, w in zip(got, n64):
            assert np.isfinite(g).all()
            worst = max(worst, float(np.abs(g - w).max()) / float(np.abs(w).max()))
    e32 = max(SC.errors(b, a, b)[1] for a, b in zip(n64, n32))
    print("%s: windowed against whole-utterance float64, e = %.3g; float32 checker %.3g from float64" % (cid, worst, e32))
    assert worst <= 1e-12, (cid, worst)


def test_cases_cover_what_they_are_there_for():
    from twvk_amd import score as S

    def windows(cid, wf=None):
        c = WC.case(cid)
        t = S.plan(c.lengths, (wf or c.windows[0]) * c.hop, c.rf, c.hop, c.slots).table
        return [int((t[:, :, S.UTT] == i).sum()) for i in range(len(c.lengths))], int((t[:, :, S.UTT] < 0).sum())
    for cid in ("w64-small", "w128-small"):
        assert windows(cid) == ([1, 1, 3], 1)
    assert WC.case("w64-ow1").lengths[0] == WC.case("w64-ow1").rf + 1
    assert windows("w128-one-cycle")[0] == [1, 3] and WC.case("w128-one-cycle").rf == 1055
    assert windows("w128-thirty-layers")[0] == [13] and WC.case("w128-thirty-layers").n_layers * 128 == 3840
    for cid in ("w64-hop32", "w128-hop32"):
        c = WC.case(cid)
        assert c.hop == 32 and [w * c.hop for w in c.windows] == [S.halo(c.rf, c.hop) + c.hop, S.halo(c.rf, c.hop) + 5 * c.hop]
    assert {(c[1], c[6]["lc"]) for c in WC.CASES} >= {(64, "fused"), (64, "staged"), (128, "fused"), (128, "staged")}
