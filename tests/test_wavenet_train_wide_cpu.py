"""Host-only side of the wide training-step tests (residual_channels = dilation_channels = 64 and 128): twv_wavenet_train_create_w's
contract -- widths, refusals, route label, parameter count, workspace size -- on every case of tests/train_wide_cases.py, and that the
export and the wide kernels are in the header, the bindings and the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import train_cases as TC
import train_wide_cases as TW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 2
OLD_TEXT = b"training is built for residual_channels = dilation_channels = 32 only: training at other widths is not built"


class _Edited(object):
    """the dims edited behind the Python model (which has refusals of its own)"""

    def __init__(self, net, **over):
        from twvk_amd import _lib
        self._dims = _lib.Dims.from_buffer_copy(net._dims)
        for k, v in over.items():
            setattr(self._dims, k, v)


@pytest.mark.parametrize("cid", TW.IDS)
def test_case_is_on_its_route_and_the_sizes_follow_the_model(cid):
    from twvk_amd import weights as Wt
    _, W, kw, want = TW.BY_ID[cid]
    route, ws, n = TW.host_route(W, kw)
    assert route["width"] == str(W) and W in (64, 128)
    assert {k: route[k] for k in want} == want, (cid, route)
    scalar = kw.get("scalar_input", True)
    specs = Wt.tensor_specs(len(kw["dil"]), W, W, S=kw.get("S", 64), Q=kw.get("Q", 256), out_channels=kw.get("out_channels", 30), scalar_input=scalar,
                            initial_filter_width=kw.get("ifw", 32), use_biases=kw.get("use_bias", True), gc_channels=kw.get("G", 32),
                            gc_cardinality=kw.get("gc_card", 2), upsample_factor=kw.get("up", TC.UP))
    assert n == sum(int(np.prod(shape)) for _, shape in specs)
    assert ws >= int(route["carve_floats"]) + n + 1024
    # what the step keeps per layer alone: X, tanh and sigmoid rows of W floats
    rows = kw["B"] * (TW.samples(kw) - 1)
    assert int(route["carve_floats"]) > 3 * len(kw["dil"]) * rows * W


def test_workspace_grows_with_the_width():
    """at the size the step is built for (30 layers, 64 x 7800) the per-layer saved arrays make the workspace, and it grows with W; in
    a five-layer toy the width-32 step's fixed-size pieces (its 256 gradient slabs per layer) outweigh them, so there only 64 < 128"""
    big = dict(TC.BIG_CASES)["configs[3] 64 x 7800"]
    ws = [TW.host_route(W, big)[1] for W in (32, 64, 128)]
    assert ws[2] > ws[1] > ws[0], ws
    assert 20e9 < 4 * ws[2] < 60e9, ws                       # "tens of GB" at width 128 (DESIGN 3c-w states the figure)
    _, _, kw, _ = TW.BY_ID["w64-small"]
    small = [TW.host_route(W, kw)[1] for W in (64, 128)]
    assert small[1] > small[0], small


def test_create_w_accepts_three_widths_and_refuses_the_rest():
    net = TW.model(64, TW.BY_ID["w64-small"][2], "cpu")
    for W in (32, 64, 128):
        rc, h, L = TW.create_w(_Edited(net, residual_channels=W, dilation_channels=W)._dims, 2, 900, 128)
        assert rc == 0, W
        assert ("width=%d" % W).encode() in L.twv_wavenet_train_route(h)
        L.twv_wavenet_train_destroy(h)
    for R, D in ((64, 32), (32, 64), (128, 64), (128, 32), (96, 96), (16, 16), (256, 256)):
        rc, h, L = TW.create_w(_Edited(net, residual_channels=R, dilation_channels=D)._dims, 2, 900, 128)
        assert rc == UNSUPPORTED and not h.value, (R, D, rc)
        assert b"32, 64 or 128 only (got %d, %d)" % (R, D) in L.twv_last_error(), (R, D)
    # a width above the caller's max_width
    rc, h, L = TW.create_w(_Edited(net, residual_channels=128, dilation_channels=128)._dims, 2, 900, 64)
    assert rc == UNSUPPORTED and b"32, 64 or 128" in L.twv_last_error()
    rc, h, L = TW.create_w(net._dims, 2, 900, 64)
    assert rc == 0 and b"width=64" in L.twv_wavenet_train_route(h)
    L.twv_wavenet_train_destroy(h)
    # max_width 32 is twv_wavenet_train_create, with its text
    for R, D in ((64, 64), (128, 128), (64, 32)):
        rc, h, L = TW.create_w(_Edited(net, residual_channels=R, dilation_channels=D)._dims, 2, 900, 32)
        assert rc == UNSUPPORTED and OLD_TEXT in L.twv_last_error(), (R, D)
    for mw in (48, 0, 256, -32):
        rc, h, L = TW.create_w(net._dims, 2, 900, mw)
        assert rc == INVALID and not h.value, mw
    assert b"max_width" in L.twv_last_error()
    from twvk_amd import _lib
    assert L.twv_wavenet_train_create_w(C.byref(net._dims), 2, 900, 128, None) == INVALID
    with pytest.raises(_lib.TwvError):
        _lib.check(INVALID)


@pytest.mark.parametrize("cid", ["small", "two-stage", "onehot-q100"])
def test_width_32_handle_is_the_one_of_train_create(cid):
    """label (carve_floats included), workspace and parameter count of a width-32 handle are the same from either export"""
    kw = TC.PATH_BY_ID[cid][1] if cid in TC.PATH_BY_ID else dict(TC.DEFAULT_CASES)[cid]
    old = TC.host_route(**kw)
    for mw in (32, 64, 128):
        new = TW.host_route(32, dict(kw), mw)
        assert new == old, (cid, mw, new, old)
    assert old[0]["width"] == "32"


def test_export_and_kernels_are_in_header_bindings_and_library():
    from twvk_amd import _lib
    name = "twv_wavenet_train_create_w"
    header = open(os.path.join(ROOT, "include", "twv_amd.h")).read()
    L = _lib.lib()
    assert re.search(r"\b%s\(" % name, header) and name in _lib.EXPORTS and hasattr(L, name)
    assert L.twv_wavenet_train_create_w.argtypes is not None and len(L.twv_wavenet_train_create_w.argtypes) == 5
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for k in ("tr_layer_wide_fwd_kernel", "tr_layer_wide_bwd1_kernel", "tr_layer_wide_bwd2_kernel", "tr_wide_frame_sum_kernel", "tr_wide_dq_kernel",
              "tr_onehot_causal_wide_bwd_kernel", "tr_views_wide_bwd_kernel"):
        assert k in nm, "the gfx950 kernel %s must be in the library" % k


def test_table_covers_what_it_is_there_for():
    seen = {(c[1], c[3]["lc"], c[3]["head"], c[3]["loss"]) for c in TW.CASES}
    assert {(64, "fused", "skinny+c2bwd", "mol<10>"), (128, "fused", "skinny+c2bwd", "mol<10>"), (64, "staged", "skinny+c2bwd", "mol<10>"),
            (128, "staged", "skinny+c2bwd", "mol<10>"), (128, "fused", "gemm", "mol<0>"), (64, "fused", "gemm", "softmax"), (128, "fused", "gemm", "softmax"),
            (64, "staged", "gemm", "softmax")} <= seen
    assert any(c[3]["nsplit"] == "1" and c[2]["B"] > 16 for c in TW.CASES)
    import torch_train_ref as R
    tensors, cfg, audio, lc, gc, q = TW.data("w64-ow1")
    assert audio.shape[1] - R.receptive_field(cfg) == 1
    assert TW.data("w128-onehot-q512-s128")[5].max() < 512 and TW.data("w64-hop32")[2].shape[1] == 40 * 32
