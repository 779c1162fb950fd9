"""Shared by the training-step tests and scripts/train_parity_report.py: the case builder, the bars, and the table of geometries that
take the kernel families the default hparams never select (tests/test_train_paths_gpu.py runs them, tests/test_train_paths_cpu.py
checks on the host that each one is on the route it is meant to cover)."""
import ctypes as C

import numpy as np

UP = (5, 5, 12)

# Bars, from the data of scripts/train_parity_report.py (profiles/r05_train_parity_report.txt: every geometry of tests/test_train_gpu.py,
# per tensor e = max|g - g64| / max|g64| for the HIP gradients and for the float32 torch model, both against the float64 torch model):
#   * wherever a float32 model has a measurable error of its own the HIP path was at most 4.1x further from float64 than the torch
#     float32 model (16 x 3600: layer4 skip kernel; full size 2.1x; MoL-branch case 1.5x) -> asserted: 8x;
#   * tensors the torch float32 model gets right to ~1e-7 (one ulp of the largest element) the HIP path gets right to 3.3e-6 at worst
#     (chunked / split-K summation orders) -> absolute floor 5e-6 (rounds 1-4 carried 2e-3 here, which would have hidden a wrong
#     bias-gradient term in a small tensor);
#   * loss: at most 10x the float32 model's own distance from float64, floor 2e-6 relative (worst seen 3.7e-7).
# The geometries of PATH_CASES below (profiles/train_paths_parity_report.txt) are held to the same three numbers.
RATIO, FLOOR, LOSS_FLOOR = 8.0, 5e-6, 2e-6


def _model(B, dil, S, use_bias, up, out_channels, ifw, G, gc_card, scalar_input, Q, device):
    import twvk_amd  # noqa: F401
    from twvk_amd.wavenet import WaveNetModel
    return WaveNetModel(B, dil, 2, 32, 32, S, quantization_channels=Q, out_channels=out_channels, use_biases=use_bias,
                        scalar_input=scalar_input, initial_filter_width=ifw, global_condition_channels=G,
                        global_condition_cardinality=gc_card, local_condition_channels=80, upsample_factor=list(up),
                        train_mode=True, device=device)


def case_data(dil, B, Tm, S=64, seed=0, scale=0.05, ls_bias=None, clip_audio=False, use_bias=True, up=UP, out_channels=30, ifw=32,
              G=32, gc_card=2, gc_ids=None, scalar_input=True, Q=256, clamp_first=0):
    """host only: (tensors, cfg for torch_train_ref, audio, lc, gc ids, quantized).  `quantized` (one-hot model only, else None) is
    the C oracle's mu_law_encode of the audio: the encoder the device quantizer is pinned to bit for bit."""
    import twvk_amd  # noqa: F401
    from twvk_amd import weights as W
    specs = W.tensor_specs(len(dil), S=S, Q=Q, out_channels=out_channels, scalar_input=scalar_input, initial_filter_width=ifw,
                           use_biases=use_bias, gc_channels=G, gc_cardinality=gc_card, upsample_factor=up)
    tensors = W.random_tensors(specs, seed=seed, scale=scale)
    nr = out_channels // 3
    if ls_bias is not None:
        tensors["wavenet/conv1d_2/bias"][2 * nr:3 * nr] = ls_bias   # log-scales: exercises the cdf_delta > 1e-5 branch
    if clamp_first:
        tensors["wavenet/conv1d_2/bias"][2 * nr:2 * nr + clamp_first] = -40.0   # below log(1e-14) = -32.2: clamped, zero gradient
    T = Tm * int(np.prod(up))
    rng = np.random.RandomState(seed + 1)
    audio = ((rng.rand(B, T) - 0.5) * 1.6).astype(np.float32)
    if clip_audio:
        audio = np.clip(audio * 1.5, -1.0, 1.0).astype(np.float32)  # some targets at +-1: the two edge branches
    lc = (rng.randn(B, Tm, 80) * 0.5).astype(np.float32)
    gc = rng.randint(0, 2, size=B).astype(np.int32)
    if gc_ids is not None:
        gc = np.asarray(gc_ids, np.int32)
        assert gc.shape == (B,) and gc.min() >= 0 and gc.max() < gc_card
    cfg = dict(dilations=dil, initial_filter_width=ifw if scalar_input else 2, use_biases=use_bias, upsample_factor=up)
    quantized = None
    if not scalar_input:
        from oracle import oracle as O
        O.build()
        cfg.update(scalar_input=False, Q=Q)
        quantized = O.mu_law_encode(audio, Q)
    return tensors, cfg, audio, lc, gc, quantized


def _model_kw(kw):
    return dict(B=kw["B"], dil=kw["dil"], S=kw.get("S", 64), use_bias=kw.get("use_bias", True), up=kw.get("up", UP),
                out_channels=kw.get("out_channels", 30), ifw=kw.get("ifw", 32), G=kw.get("G", 32), gc_card=kw.get("gc_card", 2),
                scalar_input=kw.get("scalar_input", True), Q=kw.get("Q", 256))


def host_route(**kw):
    """host only (no device is touched): twv_wavenet_train_create on the case's dims -> (route dict, workspace floats)"""
    from twvk_amd import _lib
    net = _model(device="cpu", **_model_kw(kw))
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_wavenet_train_create(C.byref(net._dims), kw["B"], kw["Tm"] * int(np.prod(kw.get("up", UP))), C.byref(h)))
    try:
        route = dict(kv.split("=", 1) for kv in L.twv_wavenet_train_route(h).decode().split())
        return route, L.twv_wavenet_train_workspace_bytes(h) // 4, L.twv_wavenet_train_param_floats(h)
    finally:
        L.twv_wavenet_train_destroy(h)


def _case6(**kw):
    """(trainer on cuda:0 with the case's weights loaded, tensors, cfg, audio, lc, gc, quantized)"""
    from twvk_amd.train import WaveNetTrainer
    tensors, cfg, audio, lc, gc, quantized = case_data(**kw)
    net = _model(device="cuda:0", **_model_kw(kw))
    tr = WaveNetTrainer(net, sample_size=audio.shape[1])
    tr.load_weights(tensors)
    return tr, tensors, cfg, audio, lc, gc, quantized


def _case(**kw):
    return _case6(**kw)[:6]


def _assert_against_float64(label, loss, got, l64, g64, l32, g32, floor=FLOOR):
    assert abs(loss - l64) <= max(10 * abs(l32 - l64), LOSS_FLOOR * abs(l64)), (label, loss, l32, l64)
    worst_e, worst_r = ("", 0.0, 0.0), ("", 0.0)
    for k in g64:
        scale = max(float(np.abs(g64[k]).max()), 1e-30)
        e_hip = float(np.abs(got[k] - g64[k]).max()) / scale
        e_t32 = float(np.abs(g32[k] - g64[k]).max()) / scale
        assert np.isfinite(got[k]).all(), k
        assert e_hip <= max(RATIO * e_t32, floor), ("%s %s: HIP %.3g vs torch-f32 %.3g (relative to the tensor's max, against float64): ratio %.1f"
                                                    % (label, k, e_hip, e_t32, e_hip / max(e_t32, 1e-30)))
        if e_hip > worst_e[1]:
            worst_e = (k, e_hip, e_t32)
        if e_hip > floor and e_hip / e_t32 > worst_r[1]:
            worst_r = (k, e_hip / e_t32)
    print("%s: loss %.7f (f64 %.7f, f32 %.7f); worst gradient tensor %s at %.2e of its max (torch f32: %.2e); worst e_hip / e_t32 above the floor: %.2f (%s)"
          % (label, loss, l64, l32, worst_e[0], worst_e[1], worst_e[2], worst_r[1], worst_r[0] or "none above the floor"))
    return worst_e, worst_r


# The geometries of tests/test_train_gpu.py (all on the fused lc route: the claim test_train_paths_cpu.py checks)
DEFAULT_CASES = [
    ("small", dict(dil=[1, 2, 4, 1, 2], B=2, Tm=3)),
    ("one-cycle", dict(dil=[1, 2, 4, 8, 16, 32, 64, 128, 256, 512], B=3, Tm=6, S=128)),
    ("mol-branches", dict(dil=[1, 2, 4, 1, 2], B=2, Tm=3, ls_bias=-4.0, clip_audio=True)),
    ("no-bias", dict(dil=[1, 2, 4], B=1, Tm=2, use_bias=False)),
    ("hop64", dict(dil=[1, 2, 4, 8], B=2, Tm=21, up=(4, 4, 4))),          # hop 64: a 32-row tile of the fused layer kernels straddles a frame edge every other tile
    ("hop32", dict(dil=[1, 2, 4], B=2, Tm=40, up=(2, 4, 4))),             # hop 32 = the tile height (the smallest hop the frame-rate lc path takes)
    ("no-bias-s128", dict(dil=[1, 2, 4], B=2, Tm=5, S=128, use_bias=False)),     # S % 128 == 0 takes the fused conv1d_2 backward; here without bias vectors
    ("s256", dict(dil=[1, 2], B=1, Tm=4, S=256)),                        # two column groups of the fused conv1d_2 backward, a ragged last row tile
]
BIG_CASES = [
    ("bench-geometry 16 x 3600", dict(dil=[2 ** i for i in range(10)] * 3, B=16, Tm=12, S=512)),
    ("configs[3] 64 x 7800", dict(dil=[2 ** i for i in range(10)] * 3, B=64, Tm=26, S=512)),
]
OTHER_DEFAULT_GEOMETRIES = [     # the remaining tests of test_train_gpu.py
    dict(dil=[1, 2, 4, 8, 1, 2, 4, 8], B=4, Tm=4), dict(dil=[1, 2, 4], B=2, Tm=2), dict(dil=[1, 2, 4, 8, 1, 2], B=3, Tm=4, seed=4),
    dict(dil=[1, 2, 4, 8, 1, 2], B=2, Tm=2, scalar_input=False, Q=256, seed=3, scale=0.1), dict(dil=[1, 2, 4, 1, 2], B=2, Tm=3, scale=0.3),
]

OW1_DIL = [1, 2, 4, 8, 16, 32, 64, 128, 12]          # receptive field 299 of one 300-sample frame: output width 1


def _r(lc, head, loss, nsplit):
    return dict(lc=lc, head=head, loss=loss, nsplit=str(nsplit))


# (id, case, the route it is meant to cover).  head: "skinny+c2bwd" = tr_skinny_nn_kernel<true> + tr_conv2_bwd_kernel, "skinny" =
# tr_skinny_nn_kernel<false> + wgrad / relu_bwd_colsum, "gemm" = rocBLAS + tr_bias_add_kernel + wgrad
PATH_CASES = [
    # the staged lc route: tr_up_fwd, tr_layer_fwd<false>, tr_layer_bwd1<false>, tr_layer_bwd2<false>, tr_up_bwd_k, tr_up_bwd_in, dU ping-pong
    ("two-stage", dict(dil=[1, 2, 4, 8], B=2, Tm=3, up=(16, 16)), _r("staged", "skinny+c2bwd", "mol<10>", 2)),
    ("four-stage", dict(dil=[1, 2, 4, 1, 2], B=3, Tm=2, up=(2, 3, 5, 10)), _r("staged", "skinny+c2bwd", "mol<10>", 3)),
    ("one-stage", dict(dil=[1, 2, 4], B=2, Tm=3, up=(64,)), _r("staged", "skinny+c2bwd", "mol<10>", 2)),
    ("hop16", dict(dil=[1, 2, 4], B=2, Tm=8, up=(2, 2, 4)), _r("staged", "skinny+c2bwd", "mol<10>", 2)),
    ("hop600", dict(dil=[1, 2, 4, 8, 16], B=2, Tm=2, up=(5, 5, 24)), _r("staged", "skinny+c2bwd", "mol<10>", 2)),
    ("hop16-no-bias", dict(dil=[1, 2], B=1, Tm=5, up=(2, 2, 4), use_bias=False), _r("staged", "skinny+c2bwd", "mol<10>", 1)),
    ("staged-one-cycle", dict(dil=[2 ** i for i in range(10)], B=3, Tm=6, up=(15, 20), S=128), _r("staged", "skinny+c2bwd", "mol<10>", 3)),
    ("staged-ow1", dict(dil=OW1_DIL, B=3, Tm=1, up=(15, 20)), _r("staged", "skinny+c2bwd", "mol<10>", 3)),
    ("ow1", dict(dil=OW1_DIL, B=2, Tm=1), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    # the output head
    ("nr1", dict(dil=[1, 2, 4], B=2, Tm=2, out_channels=3), _r("fused", "skinny+c2bwd", "mol<0>", 2)),
    ("nr5", dict(dil=[1, 2, 4], B=2, Tm=2, out_channels=15), _r("fused", "skinny+c2bwd", "mol<0>", 2)),
    ("nr21", dict(dil=[1, 2, 4], B=2, Tm=2, out_channels=63), _r("fused", "gemm", "mol<0>", 2)),
    ("nr11-s192", dict(dil=[1, 2, 4], B=2, Tm=2, out_channels=33, S=192), _r("fused", "gemm", "mol<0>", 2)),
    ("s192", dict(dil=[1, 2, 4], B=2, Tm=2, S=192), _r("fused", "skinny", "mol<10>", 2)),
    ("s320-no-bias", dict(dil=[1, 2, 4], B=2, Tm=2, S=320, use_bias=False), _r("fused", "skinny", "mol<10>", 2)),
    ("clamp", dict(dil=[1, 2, 4], B=2, Tm=2, clamp_first=5), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    # the front
    ("ifw1", dict(dil=[1, 2, 4], B=2, Tm=2, ifw=1), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    ("ifw33", dict(dil=[1, 2, 4], B=2, Tm=2, ifw=33), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    ("ifw64", dict(dil=[1, 2, 4], B=2, Tm=2, ifw=64), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    ("g8", dict(dil=[1, 2, 4], B=2, Tm=2, G=8), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    ("g64-card5", dict(dil=[1, 2, 4], B=7, Tm=2, G=64, gc_card=5, gc_ids=[0, 1, 1, 3, 3, 3, 0]), _r("fused", "skinny+c2bwd", "mol<10>", 7)),
    ("b17", dict(dil=[1, 2], B=17, Tm=1), _r("fused", "skinny+c2bwd", "mol<10>", 1)),
    # the one-hot model
    ("onehot-q100", dict(dil=[1, 2, 4], B=2, Tm=2, scalar_input=False, Q=100), _r("fused", "gemm", "softmax", 2)),
    ("onehot-q2", dict(dil=[1, 2], B=2, Tm=1, scalar_input=False, Q=2), _r("fused", "skinny+c2bwd", "softmax", 2)),
    ("onehot-q512-s128", dict(dil=[1, 2], B=2, Tm=1, scalar_input=False, Q=512, S=128), _r("fused", "gemm", "softmax", 2)),
    ("onehot-staged", dict(dil=[1, 2, 4], B=2, Tm=3, scalar_input=False, Q=256, up=(16, 16), use_bias=False), _r("staged", "gemm", "softmax", 2)),
]
PATH_IDS = [c[0] for c in PATH_CASES]
PATH_BY_ID = {c[0]: c for c in PATH_CASES}
