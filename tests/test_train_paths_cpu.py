"""Host-only side of tests/test_train_paths_gpu.py: every case of the shared table is on the route it is meant to cover (and the
geometries of tests/test_train_gpu.py are all on the fused one), the float64 checker reaches the branches the cases are there for and
agrees with its own matmul form away from the default upsampler, and the workspace is as large as what loss_grad carves from it."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import torch_train_ref as R
import train_cases as TC


@pytest.mark.parametrize("cid", TC.PATH_IDS)
def test_case_is_on_the_route_it_is_meant_to_cover(cid):
    _, kw, want = TC.PATH_BY_ID[cid]
    route, ws, n = TC.host_route(**kw)
    assert {k: route[k] for k in want} == want, (cid, route)
    assert ws >= int(route["carve_floats"]) + n + 1024


def test_every_family_of_the_dispatch_is_in_the_table():
    """lc route x head x loss kernel: what the table covers, stated (a dropped case shows here)"""
    seen = {(w["lc"], w["head"], w["loss"]) for _, _, w in TC.PATH_CASES}
    assert {("staged", "skinny+c2bwd", "mol<10>"), ("staged", "gemm", "softmax"), ("fused", "skinny+c2bwd", "mol<0>"), ("fused", "gemm", "mol<0>"),
            ("fused", "skinny", "mol<10>"), ("fused", "gemm", "softmax"), ("fused", "skinny+c2bwd", "softmax")} <= seen
    assert any(w["nsplit"] == "1" and kw["B"] > 1 for _, kw, w in TC.PATH_CASES)


def test_the_default_geometries_all_take_the_fused_lc_route():
    """the claim the path cases rest on: nothing in tests/test_train_gpu.py launches the staged kernels, mol<0> or the plain skinny head"""
    for kw in [kw for _, kw in TC.DEFAULT_CASES + TC.BIG_CASES] + TC.OTHER_DEFAULT_GEOMETRIES:
        route, _, _ = TC.host_route(**kw)
        assert route["lc"] == "fused", (kw, route)
        assert route["loss"] in ("mol<10>", "softmax") and route["head"] in ("skinny+c2bwd", "gemm"), (kw, route)
        assert route["nsplit"] == str(kw["B"]) or kw["B"] > 16, (kw, route)


# ---- branch census of the checker's mol_loss -----------------------------------------------------------------------------------
def _census(kw):
    tensors, cfg, audio, lc, gc, _ = TC.case_data(**kw)
    return R.branch_census(tensors, cfg, audio, lc, gc)


def test_clamp_case_has_clamped_and_unclamped_pairs():
    c = _census(TC.PATH_BY_ID["clamp"][1])
    assert c["clamped"] > 0 and c["unclamped"] > 0, c
    assert c["clamped"] * 2 == c["pairs"], c               # the first five of ten components, in every row
    assert _census(TC.PATH_BY_ID["nr5"][1])["clamped"] == 0


def test_mol_branches_case_reaches_both_edges_and_the_mid_pdf_branch():
    c = _census(dict(TC.DEFAULT_CASES)["mol-branches"])
    assert c["lo_edge"] > 0 and c["hi_edge"] > 0 and c["mid_pdf"] > 0 and c["cdf_delta"] > 0, c
    assert c["lo_edge"] + c["hi_edge"] + c["mid_pdf"] + c["cdf_delta"] == c["pairs"]


@pytest.mark.parametrize("cid", [c for c in TC.PATH_IDS if c.startswith("onehot")])
def test_onehot_targets_cover_the_classes(cid):
    kw = TC.PATH_BY_ID[cid][1]
    tensors, cfg, audio, lc, gc, q = TC.case_data(**kw)
    Q = kw["Q"]
    assert q.min() >= 0 and q.max() < Q
    assert len(np.unique(q[:, R.receptive_field(cfg):])) >= min(Q, 16)


# ---- the checker against its own matmul form, away from the default upsampler ---------------------------------------------------
@pytest.mark.parametrize("cid", ["two-stage", "nr21", "onehot-q100"])
def test_checker_conv_and_matmul_forms_agree_in_float64(cid):
    tensors, cfg, audio, lc, gc, q = TC.case_data(**TC.PATH_BY_ID[cid][1])
    lc_, gc_ = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64, quantized=q)
    lm, gm = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64, quantized=q, matmul_form=True)
    assert abs(lc_ - lm) <= 1e-12 * abs(lc_)
    for k in gc_:
        scale = float(np.abs(gc_[k]).max())
        assert float(np.abs(gc_[k] - gm[k]).max()) <= 1e-12 * scale, k
    last = "wavenet/dilated_stack/layer%d/dilation_layer/dense/" % (len(cfg["dilations"]) - 1)
    assert not gc_[last + "kernel"].any() and not gm[last + "kernel"].any()         # no path to the loss: exactly zero


# ---- the workspace is sized by the carve ------------------------------------------------------------------------------------------
def _carve_need(dil, B, T, up, S, O, ifw, G, Q, scalar_input):
    """loss_grad's carve, restated: every piece rounded up to 64 floats (csrc/twv_train.hip: tr_carve)"""
    NL, L, hop = len(dil), 80, int(np.prod(up))
    Tn, ow = T - 1, T - (sum(dil) + ifw)
    Rr, RT, RO, F, tpb, ZW = B * Tn, B * T, B * ow, T // hop, (Tn + 31) // 32, NL * 32
    pieces, t = [], T // hop
    for f in up:
        t *= f
        pieces.append(B * t * L)
    pieces += [RT * L] * 2 + [Rr * ifw, RT, 0 if scalar_input else 256 * 2 * Q * 32]
    pieces += [Rr * 32] * (NL + 1 + 2 * NL) + [RO * ZW] * 2 + [Rr * 64] + [Rr * 32] * 2 + [RO * S] * 3 + [RO * O] * 2 + [B * G] * 2 + [B * 64 * NL, B * 64]
    vs = 64 * (64 + L + G)
    pieces += [vs * NL, ZW * S] * 2 + [512 * 96 * 64 + 1024 * 512, 256 * 11 * 1024 * NL, 1024, 16 * max(ZW, S) * S, 2048 * 64 * 32]
    q_ls = B * F * 4 * 64
    pieces += [4 * 512, B * F * 4 * L, (q_ls + 64) * NL, RT * 4, 4 * 512, (B * tpb * 512 + 64) * NL, (q_ls + 64) * NL, B * tpb * 96 * NL, B * 64 * NL, 64 * NL]
    return sum((p + 63) // 64 * 64 for p in pieces)


SWEEP_UPS = [(300, 1, 1, 1), (1, 1, 1, 1), (5, 5, 12), (16, 16), (1, 300), (64,), (2, 1, 4), (5, 5, 24)]


@pytest.mark.parametrize("scalar_input", [True, False])
@pytest.mark.parametrize("NL", [1, 2, 64])
def test_workspace_holds_the_carve(NL, scalar_input):
    """a one-layer model with upsample factors of 1 carved past the hand-kept estimate the workspace used to be sized with (by 4.3 M
    floats at 64 x 2100 samples); the size now IS the carve, and loss_grad checks it before its first device operation"""
    dil = ([1, 2, 4, 8] * 16)[:NL]
    for up, S, B in itertools.product(SWEEP_UPS, (64, 1024), (1, 17, 64)):
        hop = int(np.prod(up))
        Tm = -(-2100 // hop)
        kw = dict(dil=dil, B=B, Tm=Tm, up=up, S=S, scalar_input=scalar_input, Q=256)
        route, ws, n = TC.host_route(**kw)
        need = _carve_need(dil, B, Tm * hop, up, S, 30 if scalar_input else 256, 32 if scalar_input else 2, 32, 256, scalar_input)
        assert int(route["carve_floats"]) == need, (kw, route, need)
        assert ws >= need + (n + 63) // 64 * 64 + 1024, (kw, ws, need, n)      # + twv_wavenet_train_l2's region of its own behind the carve


def test_default_workspace_did_not_grow():
    """BASELINE configs[3] (64 x 7800, 30 layers, S 512): the estimate this replaced asked for 3 696 327 424 floats (it now takes 3 133 278 976)"""
    route, ws, _ = TC.host_route(**dict(TC.BIG_CASES)["configs[3] 64 x 7800"])
    assert ws <= 3696327424, ws


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_create_refuses_out_channels_that_are_not_three_to_ninety_six_in_threes():
    """twv_wavenet_train_create and twv_wavenet_score_create share one set of refusals (csrc/twv_wavenet_graph.hpp): out_channels = 0
    (no mixture at all: nr_mix 0, O 0) used to pass the trainer's own check.  The dims are edited behind the Python model, which has
    refusals of its own."""
    from twvk_amd import _lib
    net = TC._model(device="cpu", **TC._model_kw(TC.PATH_BY_ID["nr5"][1]))
    L = _lib.lib()
    UNSUPPORTED = 2

    def create(**over):
        dims = _lib.Dims.from_buffer_copy(net._dims)
        for k, v in over.items():
            setattr(dims, k, v)
        h = C.c_void_p()
        return L.twv_wavenet_train_create(C.byref(dims), 2, 900, C.byref(h)), h
    for oc in (0, 31, 99):
        rc, h = create(out_channels=oc)
        assert rc == UNSUPPORTED and not h.value, oc
    rc, h = create(out_channels=96)
    assert rc == 0
    L.twv_wavenet_train_destroy(h)
