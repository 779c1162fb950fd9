"""Shared by the WaveNet scoring tests (tests/test_wavenet_score_cpu.py, tests/test_wavenet_score_gpu.py) and scripts/score_parity.py:
the case table, the builders and the float64 / float32 torch references.

A case is a LIST of utterances of unequal lengths under one model.  The weights, audio, mels and speaker ids come from
train_cases.case_data (B = the number of utterances, Tm = the longest): utterance i is the first frames[i] frames of batch entry i.
The checker is tests/torch_train_ref.py's restatement of the reference's training graph run on the WHOLE utterance in float64,
unreduced (wavenet/model.py:247-312, mixture.py:27-81); the float32 run of the same lines is the scale of round-off.

Bars.  Per sample: e = max|nll - nll64| / max|nll64| per utterance, e_hip <= max(RATIO * e_t32, FLOOR) with the training step's
RATIO = 8 and FLOOR = 5e-6 (train_cases.py): the same arithmetic family (f32 MFMA, transcendental-unit activations), and the
un-averaged gradient tensors of the training step hold to it.  Mean: |l - l64| <= max(10 |l32 - l64|, LOSS_FLOOR |l64|)."""
import ctypes as C
import functools

import numpy as np

from train_cases import FLOOR, LOSS_FLOOR, OW1_DIL, RATIO, UP, _model, case_data    # noqa: F401  (the bars are re-exported)


def _r(lc, head, loss):
    return dict(lc=lc, head=head, loss=loss)


ONE_CYCLE = [2 ** i for i in range(10)]

# (id, model / data arguments of train_cases.case_data, frames of every utterance, windows to score with (frames), slots, the route the
# case is meant to cover).  Receptive field with the default ifw = 32: 32 + sum(dil); halo R = ceil(rf / hop) * hop.
CASES = [
    # hop 300, rf 42, R = 1 frame: an utterance shorter than the window, one exactly one window, one of two windows
    ("small", dict(dil=[1, 2, 4, 1, 2]), [2, 3, 5], (3,), 2, _r("fused", "skinny", "mol<10>")),
    # ... and one whose last window is shifted back to end at T (starts 0, 2, 3 of 6 frames): five windows, an idle slot in the last batch
    ("small-shifted", dict(dil=[1, 2, 4, 1, 2], seed=2), [2, 3, 6], (3,), 2, _r("fused", "skinny", "mol<10>")),
    # rf 299 of a 300-sample frame: T = rf + 1, one scored sample
    ("ow1", dict(dil=OW1_DIL), [1, 2], (2,), 2, _r("fused", "skinny", "mol<10>")),
    ("ow1-staged", dict(dil=OW1_DIL, up=(15, 20)), [1, 2], (2,), 2, _r("staged", "skinny", "mol<10>")),
    # hop 64 (rf 47, R = 64) and hop 32 (rf 39, R = 64): window starts on the frame edges of the fused lc kernel's 32-row tiles; the
    # smallest legal window R + hop and R + 5 hop
    ("hop64", dict(dil=[1, 2, 4, 8], up=(4, 4, 4)), [7, 3, 11], (2, 6), 3, _r("fused", "skinny", "mol<10>")),
    ("hop32", dict(dil=[1, 2, 4], up=(2, 4, 4)), [9, 4, 13], (3, 7), 3, _r("fused", "skinny", "mol<10>")),
    # the materialised upsampler
    ("staged", dict(dil=[1, 2, 4, 8], up=(16, 16)), [2, 4, 3], (2,), 2, _r("staged", "skinny", "mol<10>")),
    ("staged-four", dict(dil=[1, 2, 4, 1, 2], up=(2, 3, 5, 10)), [3, 1, 4], (2,), 2, _r("staged", "skinny", "mol<10>")),
    # the loss branches: narrow mixtures (cdf_delta > 1e-5 and the pdf branch), targets at +-1 (the two edge branches); clamped log-scales
    ("mol-branches", dict(dil=[1, 2, 4, 1, 2], ls_bias=-4.0, clip_audio=True), [3, 4], (2,), 2, _r("fused", "skinny", "mol<10>")),
    ("clamp", dict(dil=[1, 2, 4], clamp_first=5), [2, 3], (2,), 2, _r("fused", "skinny", "mol<10>")),
    # the head
    ("nr1", dict(dil=[1, 2, 4], out_channels=3), [2, 3], (2,), 2, _r("fused", "skinny", "mol<0>")),
    ("nr21", dict(dil=[1, 2, 4], out_channels=63), [2, 3], (2,), 2, _r("fused", "gemm", "mol<0>")),
    ("no-bias", dict(dil=[1, 2, 4], use_bias=False), [2, 3], (2,), 2, _r("fused", "skinny", "mol<10>")),
    ("s192", dict(dil=[1, 2, 4], S=192), [2, 3], (2,), 2, _r("fused", "skinny", "mol<10>")),
    # the front
    ("ifw1", dict(dil=[1, 2, 4], ifw=1), [2, 3], (2,), 2, _r("fused", "skinny", "mol<10>")),
    ("ifw64", dict(dil=[1, 2, 4], ifw=64), [2, 3], (2,), 2, _r("fused", "skinny", "mol<10>")),
    ("g64-card5", dict(dil=[1, 2, 4], G=64, gc_card=5, gc_ids=[0, 3, 1, 3, 4]), [2, 3, 1, 4, 2], (2,), 4, _r("fused", "skinny", "mol<10>")),
    # the one-hot model
    ("onehot-q256", dict(dil=[1, 2, 4, 8, 1, 2], scalar_input=False, Q=256, seed=3, scale=0.1), [2, 3], (2,), 2, _r("fused", "gemm", "softmax")),
    ("onehot-q2", dict(dil=[1, 2], scalar_input=False, Q=2), [1, 3], (2,), 2, _r("fused", "skinny", "softmax")),
    ("onehot-q512-s128", dict(dil=[1, 2], scalar_input=False, Q=512, S=128), [1, 3], (2,), 2, _r("fused", "gemm", "softmax")),
    # ten layers, rf 1055, R = 4 frames, window = R + 2 hop = 6 frames: the halo exceeds the window's own kept share; the 9-frame
    # utterance is three windows (starts 0, 2, 3), the 6-frame one exactly one
    ("one-cycle", dict(dil=ONE_CYCLE, S=128), [6, 9], (6,), 2, _r("fused", "skinny", "mol<10>")),
    # three cycles, rf 3101, R = 11 frames: 13 windows of 12 frames, one slot
    ("thirty-layers", dict(dil=ONE_CYCLE * 3, S=512), [24], (12,), 1, _r("fused", "skinny", "mol<10>")),
]
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}
MOL_IDS = [c[0] for c in CASES if c[1].get("scalar_input", True)]


class Case(object):
    """host only: the utterance list of a table entry"""

    def __init__(self, cid):
        _, kw, frames, windows, slots, route = BY_ID[cid]
        self.id, self.kw, self.frames, self.windows, self.slots, self.route = cid, dict(kw), list(frames), tuple(windows), slots, route
        self.up = tuple(kw.get("up", UP))
        self.hop = int(np.prod(self.up))
        self.tensors, self.cfg, audio, lc, gc, quantized = case_data(B=len(frames), Tm=max(frames), **kw)
        self.audios = [audio[i, :f * self.hop].copy() for i, f in enumerate(frames)]
        self.mels = [lc[i, :f].copy() for i, f in enumerate(frames)]
        self.gcs = [int(g) for g in gc]
        self.quantized = None if quantized is None else [quantized[i, :f * self.hop].copy() for i, f in enumerate(frames)]
        import torch_train_ref as R
        self.rf = R.receptive_field(self.cfg)
        self.lengths = [f * self.hop for f in frames]

    def model_kw(self, slots=None):
        kw = self.kw
        return dict(B=slots or self.slots, dil=kw["dil"], S=kw.get("S", 64), use_bias=kw.get("use_bias", True), up=self.up,
                    out_channels=kw.get("out_channels", 30), ifw=kw.get("ifw", 32), G=kw.get("G", 32), gc_card=kw.get("gc_card", 2),
                    scalar_input=kw.get("scalar_input", True), Q=kw.get("Q", 256))

    def model(self, device, slots=None):
        return _model(device=device, **self.model_kw(slots))

    def scorer(self, window_frames=None, slots=None, device="cuda:0", tensors=None):
        from twvk_amd.score import WaveNetScorer
        sc = WaveNetScorer(self.model(device, slots), window=(window_frames or self.windows[0]) * self.hop, slots=slots or self.slots)
        sc.load_weights(tensors or self.tensors)
        return sc


@functools.lru_cache(maxsize=None)
def case(cid):
    return Case(cid)


def host_route(c, window_frames=None, slots=None):
    """host only (no device is touched): twv_wavenet_score_create on the case's dims -> (route dict, workspace bytes)"""
    from twvk_amd import _lib
    net = c.model("cpu", slots)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_wavenet_score_create(C.byref(net._dims), slots or c.slots, (window_frames or c.windows[0]) * c.hop, C.byref(h)))
    try:
        return dict(kv.split("=", 1) for kv in L.twv_wavenet_score_route(h).decode().split()), int(L.twv_wavenet_score_workspace_bytes(h))
    finally:
        L.twv_wavenet_score_destroy(h)


def ref_nll(c, audio, mel, gc, quantized=None, dtype=None, tensors=None):
    """the training graph of tests/torch_train_ref.py on ONE crop, unreduced: (len(audio) - rf,) float64 numpy"""
    import torch
    import torch.nn.functional as F
    import torch_train_ref as R
    dtype = dtype or torch.float64
    cfg = c.cfg
    with torch.no_grad():
        P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in (tensors or c.tensors).items()}
        a = torch.tensor(np.asarray(audio), dtype=dtype)[None]
        U = R.upsample(torch.tensor(np.asarray(mel), dtype=dtype)[None], [P["wavenet/upsample%d/kernel" % i] for i in range(len(cfg["upsample_factor"]))],
                       cfg["upsample_factor"])
        g = torch.tensor([int(gc)])
        if cfg.get("scalar_input", True):
            y = R.network(P, cfg, a[:, None, :-1], U, g)
            out = R.mol_loss(y, a[:, c.rf:, None])[0]
        else:
            q = torch.tensor(np.asarray(quantized))[None]
            enc = F.one_hot(q.long(), cfg["Q"]).to(dtype)
            y = R.network(P, cfg, enc[:, :-1].transpose(1, 2), U, g)
            out = F.cross_entropy(y[0], q[0, c.rf:].long(), reduction="none")
    return out.double().numpy()


@functools.lru_cache(maxsize=None)
def reference(cid):
    """([nll64 per utterance], [nll32 per utterance]) on the whole utterances: computed once, shared, never modified"""
    import torch
    c = case(cid)
    out = ([], [])
    for k, dt in enumerate((torch.float64, torch.float32)):
        for i in range(len(c.audios)):
            v = ref_nll(c, c.audios[i], c.mels[i], c.gcs[i], None if c.quantized is None else c.quantized[i], dtype=dt)
            v.setflags(write=False)
            out[k].append(v)
    return out


def errors(got, n64, n32):
    """(e_hip, e_t32): max|. - nll64| / max|nll64| of one utterance"""
    scale = max(float(np.abs(n64).max()), 1e-30)
    return float(np.abs(np.asarray(got, np.float64) - n64).max()) / scale, float(np.abs(n32 - n64).max()) / scale


def assert_per_sample(label, got, n64, n32, floor=FLOOR):
    got = np.asarray(got, np.float64)
    assert got.shape == n64.shape, (label, got.shape, n64.shape)
    assert np.isfinite(got).all(), label
    e_hip, e_t32 = errors(got, n64, n32)
    print("%s: %d positions, e_hip %.3g, e_t32 %.3g" % (label, got.size, e_hip, e_t32))
    assert e_hip <= max(RATIO * e_t32, floor), "%s: HIP %.3g vs torch-f32 %.3g (relative to max|nll64|)" % (label, e_hip, e_t32)
    return e_hip, e_t32


def means(cid):
    """(l64, l32): the mean over every scored position of the list"""
    n64, n32 = reference(cid)
    return float(np.concatenate(n64).mean()), float(np.concatenate(n32).mean())
