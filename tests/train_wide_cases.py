"""Shared by the wide training-step tests (tests/test_wavenet_train_wide_cpu.py, tests/test_wavenet_train_wide_gpu.py) and
scripts/train_parity_report.py --wide: the training step at residual_channels = dilation_channels = W in {64, 128}
(twv_wavenet_train_create_w; tr_layer_wide_fwd / bwd1 / bwd2_kernel) -- the smallest shapes at which each piece can still go wrong.

Models and data come from score_wide_cases.wide_model / wide_case_data (train_cases' recipe at width W); the checker is
torch_train_ref.loss_and_grads in float64 and float32 (width-agnostic), the bars train_cases' RATIO and LOSS_FLOOR.

FLOOR_G, the floor of the gradient bar e <= max(RATIO * e_t32, FLOOR_G): it starts from the project's FLOOR = 5e-6, measured at width
32.  It may rise only if some wide tensor fails where the float32 model is itself exact (e_t32 < 1e-7), and then to at most 2 x the
worst e_hip the width-32 step shows on the width-32 twins of these cases (a wide contraction sums up to 2.3 x as many products); the
twins' figures and the choice are line `floor_g` of profiles/wavenet_train_wide_parity.txt.  No wide tensor needed more than FLOOR."""
import ctypes as C
import functools

import numpy as np

import score_wide_cases as WC
from train_cases import FLOOR, LOSS_FLOOR, OW1_DIL, RATIO, UP    # noqa: F401  (the bars are re-exported)

FLOOR_G = FLOOR         # 5e-6: profiles/wavenet_train_wide_parity.txt, line `floor_g`
ONE_CYCLE = [2 ** i for i in range(10)]


def _r(lc, head, loss, nsplit):
    return dict(lc=lc, head=head, loss=loss, nsplit=str(nsplit))


_SMALL = dict(dil=[1, 2, 4, 1, 2], B=2, Tm=3)
_STAGED = dict(dil=[1, 2, 4, 8], up=(16, 16), B=2, Tm=3)
_HOP32 = dict(dil=[1, 2, 4], up=(2, 4, 4), B=2, Tm=40)

# (id, W, case, the route it is on)
CASES = [
    # the fused lc route, repeated dilations
    ("w64-small", 64, _SMALL, _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    ("w128-small", 128, _SMALL, _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    # the materialised upsampler: U^T dPRE, dU accumulated over the layers
    ("w64-staged", 64, _STAGED, _r("staged", "skinny+c2bwd", "mol<10>", 2)),
    ("w128-staged", 128, _STAGED, _r("staged", "skinny+c2bwd", "mol<10>", 2)),
    # hop 32 = the tile height: a frame edge in every 32-row tile (frame sums, Dbuf)
    ("w64-hop32", 64, _HOP32, _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    ("w128-hop32", 128, _HOP32, _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    # one scored row per entry: nearly every row masked
    ("w64-ow1", 64, dict(dil=OW1_DIL, B=2, Tm=1), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    # shifts across many tiles and batch entries, an odd batch
    ("w128-one-cycle", 128, dict(dil=ONE_CYCLE, B=3, Tm=6, S=128), _r("fused", "skinny+c2bwd", "mol<10>", 3)),
    ("w128-no-bias", 128, dict(dil=[1, 2, 4], B=1, Tm=2, use_bias=False), _r("fused", "skinny+c2bwd", "mol<10>", 1)),
    # gc sums, embedding scatter, ids 2 and 4 unused
    ("w64-g64-card5", 64, dict(dil=[1, 2, 4], B=7, Tm=2, G=64, gc_card=5, gc_ids=[0, 1, 1, 3, 3, 3, 0]), _r("fused", "skinny+c2bwd", "mol<10>", 7)),
    # the causal layer's gradient with N = W
    ("w128-ifw33", 128, dict(dil=[1, 2, 4], B=2, Tm=2, ifw=33), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    ("w64-ifw1", 64, dict(dil=[1, 2, 4], B=2, Tm=2, ifw=1), _r("fused", "skinny+c2bwd", "mol<10>", 2)),
    # the rocBLAS head, mol<0>
    ("w128-nr21", 128, dict(dil=[1, 2, 4], B=2, Tm=2, out_channels=63), _r("fused", "gemm", "mol<0>", 2)),
    # the one-hot model: softmax cross-entropy, the column-blocked causal backward (at Q = 512 the table fills the LDS)
    ("w64-onehot-q256", 64, dict(dil=[1, 2, 4, 8, 1, 2], B=2, Tm=2, scalar_input=False, Q=256, seed=3, scale=0.1), _r("fused", "gemm", "softmax", 2)),
    ("w128-onehot-q512-s128", 128, dict(dil=[1, 2], B=2, Tm=1, scalar_input=False, Q=512, S=128), _r("fused", "gemm", "softmax", 2)),
    ("w64-onehot-staged", 64, dict(dil=[1, 2, 4], B=2, Tm=3, scalar_input=False, Q=256, up=(16, 16), use_bias=False), _r("staged", "gemm", "softmax", 2)),
    # nsplit = 1: more entries than slabs
    ("w64-b17", 64, dict(dil=[1, 2], B=17, Tm=1), _r("fused", "skinny+c2bwd", "mol<10>", 1)),
]
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}


def model(W, kw, device):
    return WC.wide_model(W, B=kw["B"], dil=kw["dil"], S=kw.get("S", 64), use_bias=kw.get("use_bias", True), up=kw.get("up", UP),
                         out_channels=kw.get("out_channels", 30), ifw=kw.get("ifw", 32), G=kw.get("G", 32), gc_card=kw.get("gc_card", 2),
                         scalar_input=kw.get("scalar_input", True), Q=kw.get("Q", 256), device=device)


def samples(kw):
    return kw["Tm"] * int(np.prod(kw.get("up", UP)))


def create_w(dims, batch, n_samples, max_width):
    """twv_wavenet_train_create_w -> (return code, handle, library)"""
    from twvk_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    return L.twv_wavenet_train_create_w(C.byref(dims), batch, n_samples, max_width, C.byref(h)), h, L


def host_route(W, kw, max_width=128):
    """host only (no device is touched): (route dict, workspace floats, parameter floats)"""
    from twvk_amd import _lib
    rc, h, L = create_w(model(W, kw, "cpu")._dims, kw["B"], samples(kw), max_width)
    _lib.check(rc)
    try:
        route = dict(kv.split("=", 1) for kv in L.twv_wavenet_train_route(h).decode().split())
        return route, L.twv_wavenet_train_workspace_bytes(h) // 4, L.twv_wavenet_train_param_floats(h)
    finally:
        L.twv_wavenet_train_destroy(h)


@functools.lru_cache(maxsize=None)
def data(cid, width=None):
    """(tensors, cfg, audio, lc, gc, quantized) of a table case; `width`: another width (32: the case's width-32 twin)"""
    _, W, kw, _ = BY_ID[cid]
    return WC.wide_case_data(int(width or W), **kw)


@functools.lru_cache(maxsize=None)
def reference(cid, width=None):
    """(l64, g64, l32, g32): the float64 and float32 checkers, computed once, shared, never modified"""
    import torch
    import torch_train_ref as R
    tensors, cfg, audio, lc, gc, q = data(cid, width)
    l64, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, quantized=q, dtype=torch.float64)
    l32, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, quantized=q, dtype=torch.float32)
    for g in (g64, g32):
        for v in g.values():
            v.setflags(write=False)
    return l64, g64, l32, g32


def trainer(cid, width=None, **opts):
    """a fresh WaveNetTrainer on cuda:0 with the case's weights loaded"""
    from twvk_amd.train import WaveNetTrainer
    _, W, kw, _ = BY_ID[cid]
    tr = WaveNetTrainer(model(int(width or W), kw, "cuda:0"), sample_size=samples(kw), **opts)
    tr.load_weights(data(cid, width)[0])
    return tr
