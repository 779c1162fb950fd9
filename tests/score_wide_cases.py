"""Shared by the wide WaveNet scoring tests (tests/test_wavenet_score_wide_cpu.py, tests/test_wavenet_score_wide_gpu.py) and
scripts/score_parity.py --width: scoring at residual_channels = dilation_channels = W in {64, 128} (sc_layer_wide_fwd_kernel), and
the width-32 twins of the same cases (the untouched sc_layer_fwd_kernel, measured through the same views).

The table mirrors score_cases.CASES.  train_cases._model and case_data are written for width 32, so the model and the tensors are
built here from weights.tensor_specs(n_layers, W, W, ...) with the same recipe: random_tensors (sigma 0.05 unless the mirrored case
says otherwise), audio uniform in +-0.8, mel N(0, 0.5^2), speaker ids from the same generator.  The NLL checker, the error measure and
the bars are score_cases' own (ref_nll, errors, assert_per_sample; RATIO, FLOOR, LOSS_FLOOR of train_cases).

The NLL alone cannot see a wrong channel of a wide layer (one dead channel of one layer moves it by 5e-10 .. 2e-5 of max|nll|, mostly
below the bar's floor), so the tests also compare what twv_wavenet_score_view exposes: every layer's z rows (the stacked skip input ZC)
and the raw output Y against `network_mm_z`, this file's matmul-form checker that returns them.

FLOOR_Z, the floor of the z / y bar e <= max(RATIO * e_t32, FLOOR_Z): max(5e-6, 2 x the worst e_z of the width-32 kernel through the
same view on the width-32 twins); the factor 2 because a wide pre-activation sums up to 2.3 x as many products (2 * 128 + 80 against
2 * 32 + 80) and rounding grows about as the square root.  Figures: profiles/wavenet_score_wide_parity.txt, line `floor_z`."""
import ctypes as C
import functools

import numpy as np

import score_cases as SC
from train_cases import FLOOR, LOSS_FLOOR, OW1_DIL, RATIO, UP    # noqa: F401  (the bars are re-exported)

ONE_CYCLE = SC.ONE_CYCLE
FLOOR_Z = 5e-6          # profiles/wavenet_score_wide_parity.txt, line `floor_z`


def _r(lc, head, loss):
    return dict(lc=lc, head=head, loss=loss)


_SMALL = dict(dil=[1, 2, 4, 1, 2])
_STAGED = dict(dil=[1, 2, 4, 8], up=(16, 16))
_HOP32 = dict(dil=[1, 2, 4], up=(2, 4, 4))
_G64 = dict(dil=[1, 2, 4], G=64, gc_card=5, gc_ids=[0, 3, 1, 3, 4])

# (id, W, model / data arguments, frames of every utterance, windows to score with (frames), slots, route)
CASES = [
    # five windows, one shifted back to end at T, an idle slot in the last batch
    ("w64-small", 64, _SMALL, [2, 3, 6], (3,), 2, _r("fused", "skinny", "mol<10>")),
    ("w128-small", 128, _SMALL, [2, 3, 6], (3,), 2, _r("fused", "skinny", "mol<10>")),
    # the materialised upsampler: 80 more k-steps per channel block
    ("w64-staged", 64, _STAGED, [2, 4, 3], (2,), 2, _r("staged", "skinny", "mol<10>")),
    ("w128-staged", 128, _STAGED, [2, 4, 3], (2,), 2, _r("staged", "skinny", "mol<10>")),
    # hop 32 = the tile height: a 32-row tile meets a frame edge in every tile
    ("w64-hop32", 64, _HOP32, [9, 4, 13], (3, 7), 3, _r("fused", "skinny", "mol<10>")),
    ("w128-hop32", 128, _HOP32, [9, 4, 13], (3, 7), 3, _r("fused", "skinny", "mol<10>")),
    # T = rf + 1: one scored sample
    ("w64-ow1", 64, dict(dil=OW1_DIL), [1, 2], (2,), 2, _r("fused", "skinny", "mol<10>")),
    ("w128-no-bias", 128, dict(dil=[1, 2, 4], use_bias=False), [2, 3], (2,), 2, _r("fused", "skinny", "mol<10>")),
    ("w64-g64-card5", 64, _G64, [2, 3, 1, 4, 2], (2,), 4, _r("fused", "skinny", "mol<10>")),
    # the one-hot model
    ("w64-onehot-q256", 64, dict(dil=[1, 2, 4, 8, 1, 2], scalar_input=False, Q=256, seed=3, scale=0.1), [2, 3], (2,), 2, _r("fused", "gemm", "softmax")),
    ("w128-onehot-q2", 128, dict(dil=[1, 2], scalar_input=False, Q=2), [1, 3], (2,), 2, _r("fused", "skinny", "softmax")),
    ("w128-nr21", 128, dict(dil=[1, 2, 4], out_channels=63), [2, 3], (2,), 2, _r("fused", "gemm", "mol<0>")),
    # dilation 512 spans many tiles, the halo exceeds the window's kept share
    ("w128-one-cycle", 128, dict(dil=ONE_CYCLE, S=128), [6, 9], (6,), 2, _r("fused", "skinny", "mol<10>")),
    # 13 windows of 12 frames, one slot, ZW = 3840
    ("w128-thirty-layers", 128, dict(dil=ONE_CYCLE * 3, S=512), [24], (12,), 1, _r("fused", "skinny", "mol<10>")),
]
IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}


def wide_model(W, B, dil, S, use_bias, up, out_channels, ifw, G, gc_card, scalar_input, Q, device):
    import twvk_amd  # noqa: F401
    from twvk_amd.wavenet import WaveNetModel
    return WaveNetModel(B, dil, 2, W, W, S, quantization_channels=Q, out_channels=out_channels, use_biases=use_bias,
                        scalar_input=scalar_input, initial_filter_width=ifw, global_condition_channels=G,
                        global_condition_cardinality=gc_card, local_condition_channels=80, upsample_factor=list(up),
                        train_mode=True, device=device)


def wide_case_data(W, dil, B, Tm, S=64, seed=0, scale=0.05, use_bias=True, up=UP, out_channels=30, ifw=32, G=32, gc_card=2, gc_ids=None,
                   scalar_input=True, Q=256):
    """train_cases.case_data's recipe at width W: (tensors, cfg for torch_train_ref, audio, lc, gc ids, quantized)"""
    import twvk_amd  # noqa: F401
    from twvk_amd import weights as Wt
    specs = Wt.tensor_specs(len(dil), W, W, S=S, Q=Q, out_channels=out_channels, scalar_input=scalar_input, initial_filter_width=ifw,
                            use_biases=use_bias, gc_channels=G, gc_cardinality=gc_card, upsample_factor=up)
    tensors = Wt.random_tensors(specs, seed=seed, scale=scale)
    T = Tm * int(np.prod(up))
    rng = np.random.RandomState(seed + 1)
    audio = ((rng.rand(B, T) - 0.5) * 1.6).astype(np.float32)
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


class Case(object):
    """host only: the utterance list of a table entry; `width` overrides the table's (32: the case's width-32 twin).  Carries what
    score_cases.ref_nll reads (cfg, tensors, rf)."""

    def __init__(self, cid, width=None):
        _, W, kw, frames, windows, slots, route = BY_ID[cid]
        self.W = int(width or W)
        self.id = cid if width is None else "%s@%d" % (cid, self.W)
        self.kw, self.frames, self.windows, self.slots, self.route = dict(kw), list(frames), tuple(windows), slots, dict(route, width=str(self.W))
        self.up = tuple(kw.get("up", UP))
        self.hop = int(np.prod(self.up))
        self.tensors, self.cfg, audio, lc, gc, quantized = wide_case_data(self.W, B=len(frames), Tm=max(frames), **kw)
        self.audios = [audio[i, :f * self.hop].copy() for i, f in enumerate(frames)]
        self.mels = [lc[i, :f].copy() for i, f in enumerate(frames)]
        self.gcs = [int(g) for g in gc]
        self.quantized = None if quantized is None else [quantized[i, :f * self.hop].copy() for i, f in enumerate(frames)]
        import torch_train_ref as R
        self.rf = R.receptive_field(self.cfg)
        self.lengths = [f * self.hop for f in frames]
        self.n_layers = len(kw["dil"])

    def model(self, device, slots=None):
        kw = self.kw
        return wide_model(self.W, B=slots or self.slots, dil=kw["dil"], S=kw.get("S", 64), use_bias=kw.get("use_bias", True), up=self.up,
                          out_channels=kw.get("out_channels", 30), ifw=kw.get("ifw", 32), G=kw.get("G", 32), gc_card=kw.get("gc_card", 2),
                          scalar_input=kw.get("scalar_input", True), Q=kw.get("Q", 256), device=device)

    def scorer(self, window_frames=None, slots=None, device="cuda:0", tensors=None):
        from twvk_amd.score import WaveNetScorer
        sc = WaveNetScorer(self.model(device, slots), window=(window_frames or self.windows[0]) * self.hop, slots=slots or self.slots)
        sc.load_weights(tensors or self.tensors)
        return sc


@functools.lru_cache(maxsize=None)
def case(cid, width=None):
    return Case(cid, width)


def create(dims, slots, window):
    """twv_wavenet_score_create on a Dims -> (return code, handle, library)"""
    from twvk_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    return L.twv_wavenet_score_create(C.byref(dims), slots, window, C.byref(h)), h, L


def host_route(c, window_frames=None, slots=None):
    """host only: (route dict, workspace bytes, {name: (offset, rows, cols)} of twv_wavenet_score_view)"""
    from twvk_amd import _lib
    rc, h, L = create(c.model("cpu", slots)._dims, slots or c.slots, (window_frames or c.windows[0]) * c.hop)
    _lib.check(rc)
    try:
        views = {}
        for name in ("zc", "y"):
            o, r, k = C.c_longlong(), C.c_longlong(), C.c_longlong()
            _lib.check(L.twv_wavenet_score_view(h, name.encode(), C.byref(o), C.byref(r), C.byref(k)))
            views[name] = (o.value, r.value, k.value)
        return dict(kv.split("=", 1) for kv in L.twv_wavenet_score_route(h).decode().split()), int(L.twv_wavenet_score_workspace_bytes(h)), views
    finally:
        L.twv_wavenet_score_destroy(h)


def network_mm_z(P, cfg, net_in, U, gc_ids):
    """torch_train_ref.network_mm (the train-mode graph in matmuls) that also returns what scoring keeps of every layer:
    (y (B, out_w, O), [z_l[:, n_l - out_w:] (B, out_w, D) for every layer])"""
    import torch
    import torch.nn.functional as F
    import torch_train_ref as R
    dil, ifw, ub = cfg["dilations"], cfg["initial_filter_width"], cfg["use_biases"]
    rf = R.receptive_field(cfg)
    if cfg.get("scalar_input", True):
        cur = net_in[:, 0, :].unfold(1, ifw, 1) @ P["wavenet/conv1d/kernel"][:, 0, :]
    else:
        x = net_in.transpose(1, 2)
        k = P["wavenet/conv1d/kernel"]
        cur = x[:, :-1] @ k[0] + x[:, 1:] @ k[1]
    out_w = net_in.shape[2] - rf + 1
    gc = P["wavenet/gc_embedding"][gc_ids.long()]

    def b(name):
        return P[name + "/bias"] if (ub and (name + "/bias") in P) else 0.0

    total, zs = None, []
    for i, d in enumerate(dil):
        p = "wavenet/dilated_stack/layer%d/dilation_layer/" % i
        n = cur.shape[1] - d
        pre = []
        for nm in ("filter", "gate"):
            w = P[p + "conv_" + nm + "/kernel"]
            v = cur[:, :n] @ w[0] + cur[:, d:] @ w[1] + b(p + "conv_" + nm)
            v = v + (gc @ P[p + "gc_" + nm + "/kernel"][0])[:, None, :]
            v = v + U[:, :n] @ P[p + "lc_" + nm + "/kernel"][0]
            pre.append(v)
        z = torch.tanh(pre[0]) * torch.sigmoid(pre[1])
        zs.append(z[:, n - out_w:])
        sk = z[:, n - out_w:] @ P[p + "skip/kernel"][0] + b(p + "skip")
        total = sk if total is None else total + sk
        cur = cur[:, d:] + (z @ P[p + "dense/kernel"][0] + b(p + "dense"))
    c1 = F.relu(total) @ P["wavenet/conv1d_1/kernel"][0] + b("wavenet/conv1d_1")
    return F.relu(c1) @ P["wavenet/conv1d_2/kernel"][0] + b("wavenet/conv1d_2"), zs


def ref_views(c, audio, mel, gc, quantized=None, dtype=None, net=None):
    """the checker on ONE crop -> (y (len - rf, O), [z_l (len - rf, W)]) float64 numpy; `net`: another network function returning y only"""
    import torch
    import torch.nn.functional as F
    import torch_train_ref as R
    dtype = dtype or torch.float64
    cfg = c.cfg
    with torch.no_grad():
        P = {k: torch.tensor(np.asarray(v), dtype=dtype) for k, v in c.tensors.items()}
        a = torch.tensor(np.asarray(audio), dtype=dtype)[None]
        U = R.upsample(torch.tensor(np.asarray(mel), dtype=dtype)[None], [P["wavenet/upsample%d/kernel" % i] for i in range(len(cfg["upsample_factor"]))],
                       cfg["upsample_factor"])
        g = torch.tensor([int(gc)])
        if cfg.get("scalar_input", True):
            net_in = a[:, None, :-1]
        else:
            net_in = F.one_hot(torch.tensor(np.asarray(quantized))[None].long(), cfg["Q"]).to(dtype)[:, :-1].transpose(1, 2)
        if net is not None:
            return net(P, cfg, net_in, U, g)[0].double().numpy(), None
        y, zs = network_mm_z(P, cfg, net_in, U, g)
    return y[0].double().numpy(), [z[0].double().numpy() for z in zs]


@functools.lru_cache(maxsize=None)
def reference(cid, width=None):
    """([nll64 per utterance], [nll32 per utterance]) on the whole utterances: computed once, shared, never modified"""
    import torch
    c = case(cid, width)
    out = ([], [])
    for k, dt in enumerate((torch.float64, torch.float32)):
        for i in range(len(c.audios)):
            v = SC.ref_nll(c, c.audios[i], c.mels[i], c.gcs[i], None if c.quantized is None else c.quantized[i], dtype=dt)
            v.setflags(write=False)
            out[k].append(v)
    return out


def means(cid, width=None):
    n64, n32 = reference(cid, width)
    return float(np.concatenate(n64).mean()), float(np.concatenate(n32).mean())


def first_batch(c, window_frames=None, slots=None):
    """the first window batch of the case's plan: (slots, 5) rows"""
    from twvk_amd import score as S
    return S.plan(c.lengths, (window_frames or c.windows[0]) * c.hop, c.rf, c.hop, slots or c.slots).table[0]


def view_errors(c, sc, rows):
    """after sc.run on the batch `rows`: the views against the checker on every live slot's crop.
    -> ({layer: (e_hip, e_t32)}, {slot: (e_hip, e_t32)} for y); e = max|. - .64| / max|.64|, per layer over the live slots, per slot for y"""
    import torch
    zc, yv = sc.view("zc").cpu().numpy().astype(np.float64), sc.view("y").cpu().numpy().astype(np.float64)
    ow, W, NL = sc.width, c.W, c.n_layers
    assert zc.shape == (sc.slots * ow, NL * W) and yv.shape[0] == sc.slots * ow
    dz, dz32, mz = np.zeros(NL), np.zeros(NL), np.zeros(NL)
    ey = {}
    for s, (u, start, n, _, _) in enumerate(rows):
        if u < 0:
            continue
        q = None if c.quantized is None else c.quantized[u][start:start + n]
        crop = (c.audios[u][start:start + n], c.mels[u][start // c.hop:(start + n) // c.hop], c.gcs[u], q)
        y64, z64 = ref_views(c, *crop)
        y32, z32 = ref_views(c, *crop, dtype=torch.float32)
        have = n - c.rf
        assert y64.shape[0] == have
        for l in range(NL):
            got = zc[s * ow:s * ow + have, l * W:(l + 1) * W]
            assert np.isfinite(got).all(), (c.id, s, l)
            dz[l] = max(dz[l], float(np.abs(got - z64[l]).max()))
            dz32[l] = max(dz32[l], float(np.abs(z32[l] - z64[l]).max()))
            mz[l] = max(mz[l], float(np.abs(z64[l]).max()))
        got = yv[s * ow:s * ow + have]
        assert np.isfinite(got).all(), (c.id, s)
        scale = float(np.abs(y64).max())
        ey[s] = (float(np.abs(got - y64).max()) / scale, float(np.abs(y32 - y64).max()) / scale)
    return {l: (dz[l] / mz[l], dz32[l] / mz[l]) for l in range(NL)}, ey


def assert_views(label, ez, ey, floor=None):
    floor = FLOOR_Z if floor is None else floor
    wz = max(ez.values(), key=lambda v: v[0])
    wy = max(ey.values(), key=lambda v: v[0])
    print("%s: z worst layer e_hip %.3g (e_t32 %.3g), y worst slot e_hip %.3g (e_t32 %.3g)" % (label, wz[0], wz[1], wy[0], wy[1]))
    for l, (e_hip, e_t32) in ez.items():
        assert e_hip <= max(RATIO * e_t32, floor), "%s layer %d z: HIP %.3g vs torch-f32 %.3g (of the layer's max|z|, against float64)" % (label, l, e_hip, e_t32)
    for s, (e_hip, e_t32) in ey.items():
        assert e_hip <= max(RATIO * e_t32, floor), "%s slot %d y: HIP %.3g vs torch-f32 %.3g (of max|y|, against float64)" % (label, s, e_hip, e_t32)
    return wz, wy
