"""-m gpu: the Tacotron training-mode graph on the device -- batch-statistics batch norm in the encoder / post-net passes
(twv_tacotron_cbhg_grad_set_mode), the passes' forward and backward halves as calls of their own, the dropout-mask generator, the
moving-average update and TacotronTrainer(training=True) -- against tests/torch_tacotron_trainmode_ref.py in float64 under the project's
gradient bar (tests/train_cases.py RATIO / FLOOR: per tensor at most 8 x the float32 autograd run's own distance from float64, floor 5e-6
of the tensor's maximum), and the exact properties of the mode.

Per-utterance independence is NOT a property of this mode: the statistics are taken over all N * T rows, so an utterance's outputs depend
on the whole batch (tests/test_tacotron_cbhg_grad_gpu.py holds the inference mode to it).

The cases are tests/tacotron_trainmode_cases.py, whose conditions tests/test_tacotron_trainmode_cpu.py proves; every case's device passes and
checker passes are computed once and shared."""
import functools

import numpy as np
import pytest

from helpers import assert_bar, first_mismatch, run_grad_handle, same_outputs
from tacotron_trainmode_cases import (CASES, MARGIN, SMALL, STEP_CASES, STEP_SEED, TWENTY_CASES, TWENTY_LR0, TWENTY_MODE, TWENTY_STEPS, ZERO_GRADIENTS,
                                      checker_trajectory, hparams, host_case, step_case, step_conditions)
from train_cases import FLOOR, RATIO

pytestmark = pytest.mark.gpu

RTOL = 5e-5          # float32 kernel vs float64 restatement, per output, relative to its maximum
STEP_ATOL = 2e-6     # tests/test_tacotron_train_gpu.py: the updated variables against clip + Adam in float64, at lr = 1e-3
INFERENCE, BATCH = 0, 1


def _stats_by_name(m, flat, which):
    return {k: v.cpu().numpy() for k, v in m._split_stats(flat, which).items()}


class _Case(object):
    """a host case with its model on the device and the C entries on its inputs; mode BATCH unless told otherwise"""

    def __init__(self, h):
        import torch
        from twvk_amd.tacotron import Tacotron
        self.h, self.torch = h, torch
        self.m = Tacotron(h.hp, num_speakers=h.speakers)
        self.m.load_weights(h.w)

    def _run(self, which, N, t, poison, call):
        def check_route(route):
            assert route["kernel"] == "cg_bigru" and route["side"] == ("post" if which else "encoder"), route
        return run_grad_handle(self.m, "twv_tacotron_cbhg_grad", (which, N, t), check_route, poison, call)

    def _set_mode(self, g, mode, m=None):
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr
        m = m or self.m
        _lib.check(m._L.twv_tacotron_cbhg_grad_set_mode(g, mode, _ptr(m.training_vector()) if mode == BATCH else None))

    def _stats(self, g, new, out):
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream
        out["stats"] = new(self.m._L.twv_tacotron_cbhg_grad_batch_stats_floats(g))
        _lib.check(self.m._L.twv_tacotron_cbhg_grad_batch_stats(g, _ptr(out["stats"]), _stream()))

    def encoder(self, d_memory=None, mode=BATCH, split=False, poison=False, model=None):
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream, encoder_grad_layout
        h, torch = self.h, self.torch
        m = model or self.m
        dev = m.device
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        tok, ln, bh, init, dm = up(h.tok), up(h.ln), up(h.bh), up(h.init), up(h.d_memory if d_memory is None else d_memory)
        m1, m2 = (up(h.masks[0]), up(h.masks[1])) if h.masks is not None else (None, None)
        L = m._L

        def call(g, ws, status, new):
            memory, grad = new(h.N, h.T, dm.shape[2]), new(m._blob.numel())
            d_bh, d_init = (new(h.N, bh.shape[1]), new(h.N, init.shape[1])) if bh is not None else (None, None)
            self._set_mode(g, mode, m)
            if split:
                _lib.check(L.twv_tacotron_encoder_grad_forward(g, _ptr(m._blob), _ptr(tok), _ptr(ln), _ptr(bh), _ptr(init), _ptr(m1), _ptr(m2), _ptr(ws),
                                                               _ptr(status), _stream(), _ptr(memory)))
                _lib.check(L.twv_tacotron_encoder_grad_backward(g, _ptr(m._blob), _ptr(tok), _ptr(ln), _ptr(dm), _ptr(ws), _ptr(status), _stream(),
                                                                _ptr(grad), _ptr(d_bh), _ptr(d_init)))
            else:
                _lib.check(L.twv_tacotron_encoder_grad_run(g, _ptr(m._blob), _ptr(tok), _ptr(ln), _ptr(bh), _ptr(init), _ptr(m1), _ptr(m2), _ptr(dm),
                                                           _ptr(ws), _ptr(status), _stream(), _ptr(memory), _ptr(grad), _ptr(d_bh), _ptr(d_init)))
            out = {"memory": memory, "blob": grad}
            if bh is not None:
                out["d_before_highway"], out["d_rnn_init"] = d_bh, d_init
            if mode == BATCH:
                self._stats(g, new, out)
            return out
        out = self._run(0, h.N, h.T, poison, call)
        return self._named(out, encoder_grad_layout(m.specs))

    def postnet(self, d_linear=None, mode=BATCH, split=False, poison=False, model=None):
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream, postnet_grad_layout
        h, torch = self.h, self.torch
        m = model or self.m
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(m.device)
        mel, dl = up(h.mel), up(h.d_linear if d_linear is None else d_linear)
        L = m._L

        def call(g, ws, status, new):
            lin, grad, d_mel = new(h.N, h.TO, dl.shape[2]), new(m._blob.numel()), new(h.N, h.TO, mel.shape[2])
            self._set_mode(g, mode, m)
            if split:
                _lib.check(L.twv_tacotron_postnet_grad_forward(g, _ptr(m._blob), _ptr(mel), _ptr(ws), _ptr(status), _stream(), _ptr(lin)))
                _lib.check(L.twv_tacotron_postnet_grad_backward(g, _ptr(m._blob), _ptr(mel), _ptr(dl), _ptr(ws), _ptr(status), _stream(), _ptr(grad),
                                                                _ptr(d_mel)))
            else:
                _lib.check(L.twv_tacotron_postnet_grad_run(g, _ptr(m._blob), _ptr(mel), _ptr(dl), _ptr(ws), _ptr(status), _stream(), _ptr(lin),
                                                           _ptr(grad), _ptr(d_mel)))
            out = {"linear": lin, "blob": grad, "d_mel": d_mel}
            if mode == BATCH:
                self._stats(g, new, out)
            return out
        out = self._run(1, h.N, h.TO, poison, call)
        return self._named(out, postnet_grad_layout(m.specs))

    def _named(self, out, layout):
        """the tensors by name: in batch mode a batch norm's slot holds (d_gamma, d_beta) themselves"""
        for name, off, shp in layout:
            out[name] = out["blob"][off:off + int(np.prod(shp))].reshape(shp)
        return out

    @functools.lru_cache(maxsize=None)
    def encoder_hip(self):
        return self.encoder()

    @functools.lru_cache(maxsize=None)
    def postnet_hip(self):
        return self.postnet()


@functools.lru_cache(maxsize=None)
def _case(name):
    import torch
    assert torch.cuda.is_available()
    return _Case(host_case(name))


def _assert_zero_gradient(label, got, g64, g32, bias):
    """the second projection's bias: its gradient is exactly zero (the batch norm behind it removes a constant), so it is held to the floor
    scaled by the tensor the same delta feeds -- the convolution's kernel"""
    kernel = bias[:-len("bias")] + "kernel"
    bound = max(RATIO * float(np.abs(g32[bias]).max()), FLOOR * float(np.abs(g64[kernel]).max()))
    worst = float(np.abs(got[bias]).max())
    print("%s %s: max|g_hip| %.3e, max|g_t32| %.3e, max|g_64| %.3e, max|d kernel_64| %.3e, bound %.3e"
          % (label, bias, worst, float(np.abs(g32[bias]).max()), float(np.abs(g64[bias]).max()), float(np.abs(g64[kernel]).max()), bound))
    assert np.isfinite(got[bias]).all() and worst <= bound, (label, bias, worst, bound)


def _assert_side(label, h, got, checker, which, fwd):
    out64, g64, rec, s64 = checker("float64")
    assert rec["relu_margin"] > MARGIN and rec["pool_gap"] > MARGIN, rec["relu_margin"]
    _, g32, _, s32 = checker("float32")
    bias = "%s_cbhg/proj_2/conv1d/bias" % which
    assert bias in ZERO_GRADIENTS
    rest = {k: v for k, v in g64.items() if k != bias}
    assert_bar(label, got, rest, g32)
    _assert_zero_gradient(label, got, g64, g32, bias)
    scale = float(np.abs(out64).max())
    assert float(np.abs(got[fwd] - out64).max()) <= RTOL * scale
    return s64, s32


@pytest.mark.parametrize("name", sorted(CASES))
def test_encoder_gradients_and_statistics_meet_the_bar(name):
    c = _case(name)
    h = c.h
    got = c.encoder_hip()
    s64, s32 = _assert_side(name + " encoder", h, got, h.encoder_checker, "encoder", "memory")
    assert_bar(name + " encoder statistics", _stats_by_name(c.m, c.torch.from_numpy(got["stats"]), "encoder"), s64, s32)
    assert not got["embedding"][0].any()
    for n, ln in enumerate(h.ln):
        assert not got["memory"][n, ln:].any() and got["memory"][n, :ln].any(), (name, n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_postnet_gradients_and_statistics_meet_the_bar(name):
    c = _case(name)
    got = c.postnet_hip()
    s64, s32 = _assert_side(name + " post", c.h, got, c.h.postnet_checker, "post", "linear")
    assert_bar(name + " post statistics", _stats_by_name(c.m, c.torch.from_numpy(got["stats"]), "post"), s64, s32)


@pytest.mark.parametrize("name", ["A-masked-tails", "H-odd-channels", "J-chunks", "K-one-row"])
def test_forward_is_the_inference_forward_at_the_batch_statistics_bit_for_bit(name):
    """a model whose moving statistics are the float32 batch statistics the device reported: its inference-mode recording forward gives the
    batch-mode forward's memory / linear, the same bits (the pair is derived and applied in the same rounding sequence in both modes)"""
    from twvk_amd.tacotron import Tacotron
    c = _case(name)
    h = c.h
    w = dict(h.w)
    for which, got in (("encoder", c.encoder_hip()), ("post", c.postnet_hip())):
        for k, s in _stats_by_name(c.m, c.torch.from_numpy(got["stats"]), which).items():
            assert (s[1] >= 0.0).all()
            w[k] = np.concatenate([np.asarray(h.w[k], np.float32)[:2], s]).astype(np.float32)
    m2 = Tacotron(h.hp, num_speakers=h.speakers)
    m2.load_weights(w)
    assert first_mismatch(c.encoder(mode=INFERENCE, model=m2)["memory"], c.encoder_hip()["memory"]) is None
    assert first_mismatch(c.postnet(mode=INFERENCE, model=m2)["linear"], c.postnet_hip()["linear"]) is None
    # and the moving statistics the case came with give another forward
    assert first_mismatch(c.encoder(mode=INFERENCE)["memory"], c.encoder_hip()["memory"]) is not None


def test_one_row_is_exact():
    """R = N * T = 1: every variance is 0 and every mean the value itself, so xhat = 0 -- every kernel and bias gradient in front of a batch
    norm and every d_gamma is exactly zero, d_beta is the incoming cotangent, the CBHG's d_x is the residual's share alone.  (A batch norm's
    OUTPUT, a * inv + (beta - a * inv) in float32, is beta up to the rounding of beta - a * inv on the grid of a * inv: it is held to the
    float64 checker, whose batch norms give beta, by the output bound of the parity tests above.)"""
    c = _case("K-one-row")
    h = c.h
    enc, post = c.encoder_hip(), c.postnet_hip()
    for which, got, names in (("encoder", enc, h.enc_names), ("post", post, h.post_names)):
        for k, s in _stats_by_name(c.m, c.torch.from_numpy(got["stats"]), which).items():
            assert not s[1].any(), k                        # the variance
        for k in names:
            if "/conv_bank/" in k or "/proj_" in k:
                if k.endswith("batch_normalization"):       # d_gamma; and d_beta = the incoming cotangent, zero in front of proj_2
                    assert not got[k][0].any() and got[k][1].any() == ("/proj_2/" in k), k
                else:
                    assert not got[k].any(), k
    # nothing reaches the prenet or the embedding but through the residual: d_x = d(highway input) = proj_2's d_beta = d_before_highway
    assert first_mismatch(enc["encoder_cbhg/proj_2/batch_normalization"][1], enc["d_before_highway"][0]) is None
    assert first_mismatch(post["post_cbhg/proj_2/batch_normalization"][1], post["d_mel"][0, 0]) is None
    assert enc["d_before_highway"].any() and post["d_mel"].any()


def test_two_runs_give_the_same_bits_also_on_nan_filled_scratch():
    for name in ("A-masked-tails", "I-dropout-masks", "J-chunks"):
        c = _case(name)
        for first, run in ((c.encoder_hip(), c.encoder), (c.postnet_hip(), c.postnet)):
            same_outputs(first, run(), name + " second run")
            poisoned = run(poison=True, split=True)
            assert all(np.isfinite(v).all() for v in poisoned.values()), name
            same_outputs(first, poisoned, name + " NaN-filled workspace and outputs, forward and backward as two calls")


def test_linear_in_the_cotangent():
    c = _case("A-masked-tails")
    h = c.h
    for one, two, zero, fwd in ((c.encoder_hip(), c.encoder(d_memory=2.0 * h.d_memory), c.encoder(d_memory=np.zeros_like(h.d_memory)), "memory"),
                                (c.postnet_hip(), c.postnet(d_linear=2.0 * h.d_linear), c.postnet(d_linear=np.zeros_like(h.d_linear)), "linear")):
        for k in one:
            if k in (fwd, "stats"):
                assert first_mismatch(one[k], two[k]) is None and first_mismatch(one[k], zero[k]) is None, k
            else:
                assert first_mismatch(2.0 * one[k], two[k]) is None, k
                assert not zero[k].any(), k


@pytest.mark.parametrize("name", ["A-masked-tails", "I-dropout-masks", "E-single-speaker"])
def test_inference_mode_through_the_halves_is_the_run_bit_for_bit(name):
    """on the inputs of tests/tacotron_cbhg_grad_cases.py: forward + backward as two calls against *_run, and the decoder's halves too"""
    import torch
    import tacotron_cbhg_grad_cases as CC
    c = _Case(CC.host_case(name))
    h, m = c.h, c.m
    same_outputs(c.encoder(mode=INFERENCE), c.encoder(mode=INFERENCE, split=True, poison=True), name + " encoder")
    same_outputs(c.postnet(mode=INFERENCE), c.postnet(mode=INFERENCE, split=True, poison=True), name + " post net")
    m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=True)
    d_mel = (np.random.RandomState(3).randn(*h.tgt.shape) / h.tgt.size).astype(np.float32)
    run = [t.cpu().numpy() for t in m._decoder_grad_blob(d_mel)]
    mel = m.decoder_grad_forward()
    halves = [t.cpu().numpy() for t in m.decoder_grad_backward(d_mel)] + [mel.cpu().numpy()]
    for a, b in zip(run, halves):
        assert first_mismatch(a, b) is None
    with torch.cuda.device(m.device):
        torch.cuda.synchronize()


# ---------------------------------------------------------------- masks and moving statistics
def test_masks_are_the_numpy_restatement_and_differ_by_site_and_step():
    from twvk_amd.tacotron import DROPOUT_SITES, dropout_mask_numpy
    m = _case("A-masked-tails").m
    n = 3 * 19 * 128
    assert n >= 4096
    masks = {}
    for step in (0, 1):
        for site in range(4):
            got = m.dropout_mask((3, 19, 128), 11, step, site).cpu().numpy()
            assert first_mismatch(got.reshape(-1), dropout_mask_numpy(n, 11, step, site)) is None, (step, site)
            assert set(np.unique(got)) == {0.0, 2.0}
            kept = float((got != 0.0).mean())
            print("step %d site %d: kept %.4f of %d" % (step, site, kept, n))
            assert abs(kept - 0.5) <= 5.0 * np.sqrt(0.25 / n), (step, site, kept)
            masks[(step, site)] = got
    keys = sorted(masks)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            differ = float((masks[a] != masks[b]).mean())
            assert abs(differ - 0.5) <= 5.0 * np.sqrt(0.25 / n), (a, b, differ)
    assert first_mismatch(m.dropout_mask((5, 7), 11, 0, "decoder_prenet_1").cpu().numpy().reshape(-1), dropout_mask_numpy(35, 11, 0, DROPOUT_SITES["decoder_prenet_1"])) is None
    other_seed = m.dropout_mask((3, 19, 128), 12, 0, 0).cpu().numpy()
    assert abs(float((other_seed != masks[(0, 0)]).mean()) - 0.5) <= 5.0 * np.sqrt(0.25 / n)
    for rate in (0.0, 0.25):
        got = m.dropout_mask((n,), 11, 0, 0, rate).cpu().numpy()
        assert first_mismatch(got, dropout_mask_numpy(n, 11, 0, 0, rate)) is None
        assert abs(float((got != 0.0).mean()) - (1.0 - rate)) <= 5.0 * np.sqrt(rate * (1.0 - rate) / n)


@pytest.mark.parametrize("name", ["A-masked-tails", "H-odd-channels"])
def test_moving_update_and_batch_gradient_convert(name):
    import torch
    import torch_tacotron_trainmode_ref as TM
    from twvk_amd import _lib
    from twvk_amd.tacotron import _grad_layout, _ptr, _stream, flatten_variables, moving_average_update, training_layout
    c = _case(name)
    h, m = c.h, c.m
    enc, post = c.encoder_hip(), c.postnet_hip()
    var0 = flatten_variables(m.specs, h.w)
    with torch.cuda.device(m.device):
        var = torch.from_numpy(var0).to(m.device)
        se, sp = torch.from_numpy(enc["stats"]).to(m.device), torch.from_numpy(post["stats"]).to(m.device)
        _lib.check(m._L.twv_tacotron_moving_update(m._h, _ptr(var), _ptr(se), _ptr(sp), 0.99, _stream()))
        g = np.random.RandomState(5).randn(m._blob.numel()).astype(np.float32)
        gb, out = torch.from_numpy(g).to(m.device), torch.full_like(var, float("nan"))
        _lib.check(m._L.twv_tacotron_grad_convert_batch(m._h, _ptr(gb), _ptr(out), _stream()))
        torch.cuda.synchronize()
    got, conv = var.cpu().numpy(), out.cpu().numpy()
    stats = dict(_stats_by_name(m, torch.from_numpy(enc["stats"]), "encoder"), **_stats_by_name(m, torch.from_numpy(post["stats"]), "post"))
    blob_at = {n: (off, shp) for n, off, shp in _grad_layout(m.specs, lambda i, n: True)}
    worst, seen = 0.0, 0
    for k, off, shp in training_layout(m.specs):
        mine, was = got[off:off + int(np.prod(shp))].reshape(shp), var0[off:off + int(np.prod(shp))].reshape(shp)
        boff, bshp = blob_at[k]
        src = g[boff:boff + int(np.prod(bshp))].reshape(bshp)
        cv = conv[off:off + int(np.prod(shp))].reshape(shp)
        if k.endswith("batch_normalization"):
            seen += 1
            assert first_mismatch(mine[:2], was[:2]) is None, k
            assert first_mismatch(mine[2:], moving_average_update(was[2:], stats[k])) is None, k
            want = TM.moving_average(was[2:], stats[k])
            worst = max(worst, float(np.abs(mine[2:] - want).max()) / float(np.abs(want).max()))
            assert (mine[2:] != was[2:]).any(), k
            assert first_mismatch(cv[:2], src) is None and not cv[2:].any() and not np.signbit(cv[2:]).any(), k
        else:
            assert first_mismatch(mine, was) is None, k
            assert first_mismatch(cv, src) is None, k
    print("%s: moving statistics against the float64 formula, worst %.3e of a tensor's maximum" % (name, worst))
    assert seen == len(stats) and worst <= 1e-6, worst


# ---------------------------------------------------------------- the training-mode step
def _trainer(h, lr0, mode, training=True, seed=STEP_SEED, randomly_initialized=True, w=None):
    from twvk_amd.tacotron import Tacotron
    from twvk_amd.tacotron_train import TacotronTrainer
    hp = hparams(max_iters=8, **dict(SMALL, tacotron_initial_learning_rate=lr0, decay_learning_rate_mode=mode, **dict(STEP_CASES, **TWENTY_CASES)[h.name][5]))
    m = Tacotron(hp, num_speakers=h.speakers)
    m.load_weights(h.w if w is None else w)
    return TacotronTrainer(m, randomly_initialized=randomly_initialized, training=training, seed=seed), (h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, h.coeff)


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_one_training_mode_step(name):
    import torch_tacotron_speaker_grad_ref as SG
    import torch_tacotron_trainmode_ref as TM
    from twvk_amd.tacotron import Tacotron, flatten
    h = step_case(name)
    ok, fig = step_conditions(h)
    assert ok, fig
    t, batch = _trainer(h, 1e-3, 1)
    m = t.model
    before = t.variables()
    inferred = m.infer(h.tok, h.ln, h.spk)[0].cpu().numpy()
    losses = t.loss_and_gradients(*batch)
    raw = t.gradients()
    # the device's masks are the restatement's, which the checker was fed
    for got, want in zip(t.last_masks, h.step_masks()):
        assert first_mismatch(got.cpu().numpy(), want) is None
    hp = h.hp
    res = {d: TM.variable_vjp(h.w, h.specs, h.dims, h.tok, h.ln, h.spk, h.at, h.tgt, h.lin_tgt, h.coeff, hp.prioritize_loss, hp.sample_rate, hp.num_freq,
                              masks=h.step_masks(), dtype=getattr(__import__("torch"), d)) for d in ("float64", "float32")}
    l64, g64, _, s64 = res["float64"]
    g32 = res["float32"][1]
    named = {k: (v[:2] if k.endswith("batch_normalization") else v) for k, v in raw.items()}
    assert abs(losses["loss"] - l64) <= 1e-4 * abs(l64), (losses["loss"], l64)
    want_g = {k: g64[k] for k in named if k not in ZERO_GRADIENTS}
    assert set(named) == set(n for n, _ in h.specs)
    assert_bar(name + " training-mode variables", named, want_g, g32)
    for bias in ZERO_GRADIENTS:
        _assert_zero_gradient(name, named, g64, g32, bias)
    for k, v in raw.items():
        if k.endswith("batch_normalization"):
            assert not v[2:].any(), k
    used = t.apply_gradients()
    lr = SG.learning_rate(1e-3, 1, 1, True)
    assert used == pytest.approx(lr, rel=1e-12) and t.global_step == 1
    after = t.variables()
    zeros = {k: np.zeros(np.shape(v)) for k, v in before.items()}
    want, _, _, norm, _ = SG.train_step(before, raw, zeros, zeros, 1, lr, hp.adam_beta1, hp.adam_beta2)
    worst = max((float(np.abs(after[k][:2].astype(np.float64) - want[k][:2]).max()) if k.endswith("batch_normalization")
                 else float(np.abs(after[k].astype(np.float64) - want[k]).max()), k) for k in want)
    print("%s: gradient norm %.4f, worst |variable - checker| %.3e (%s), bar %.3e" % (name, norm, worst[0], worst[1], STEP_ATOL * lr / 1e-3))
    assert worst[0] <= STEP_ATOL * (lr / 1e-3), worst
    worst_m = 0.0
    for k, s in s64.items():
        mv = TM.moving_average(before[k][2:], s)
        worst_m = max(worst_m, float(np.abs(after[k][2:] - mv).max()) / float(np.abs(mv).max()))
        assert (after[k][2:] != before[k][2:]).any(), k
    print("%s: moving statistics against the float64 formula on the float64 checker's statistics: worst %.3e of a tensor's maximum" % (name, worst_m))
    assert worst_m <= 1e-6, worst_m
    assert first_mismatch(m._blob.cpu().numpy(), flatten(m.specs, after)) is None
    for k in after:
        if k.endswith("batch_normalization"):
            assert first_mismatch(np.asarray(m._bn_raw[k], np.float32), after[k]) is None, k
    now = m.infer(h.tok, h.ln, h.spk)[0].cpu().numpy()
    assert first_mismatch(now, inferred) is not None
    fresh = Tacotron(m._hparams, num_speakers=h.speakers)
    fresh.load_weights(after)
    assert first_mismatch(fresh.infer(h.tok, h.ln, h.spk)[0].cpu().numpy(), now) is None
    # the evaluation graph's gradients after the step read the refreshed moving statistics
    m.forward_targets(*batch[:4], teacher_forced=True)
    ev = m.loss_gradients(batch[4], batch[5])
    fresh.forward_targets(*batch[:4], teacher_forced=True)
    ev2 = fresh.loss_gradients(batch[4], batch[5])
    for k in ev:
        assert first_mismatch(ev[k].cpu().numpy(), ev2[k].cpu().numpy()) is None, k
    # a second trainer through step(): the same bits; another seed: other masks, another loss
    t2, _ = _trainer(h, 1e-3, 1)
    assert t2.step(*batch) == losses
    same_outputs(after, t2.variables(), name + " second trainer")
    t3, _ = _trainer(h, 1e-3, 1, seed=STEP_SEED + 1)
    assert t3.step(*batch)["loss"] != losses["loss"]


def test_twenty_training_mode_steps_and_a_restore(tmp_path):
    """Twenty steps on a fixed batch against the float64 checker's own twenty steps (run on the host, masks from the restatement).  The
    device's loss and gradients agree with the checker AT THE SAME VARIABLES to the bars of the tests above, but the two runs do not keep the
    same variables: each update is held to STEP_ATOL * lr / 1e-3 per variable (tests/test_tacotron_train_gpu.py), so after k updates a
    variable may stand k * STEP_ATOL away, and to first order the loss moves by at most that times the sum of |d loss / d variable| --
    taken from the float64 checker's gradient at its twentieth step.  That is the margin; the figures are printed, and recorded in
    profiles/tacotron_trainmode_parity.txt."""
    from twvk_amd.tacotron import Tacotron
    from twvk_amd.tacotron_train import TacotronTrainer
    name = sorted(TWENTY_CASES)[0]
    h = step_case(name)
    t, batch = _trainer(h, TWENTY_LR0, TWENTY_MODE, randomly_initialized=False)
    losses = [t.step(*batch)["loss"] for _ in range(TWENTY_STEPS)]
    l64, g1 = checker_trajectory(name)
    margin = TWENTY_STEPS * STEP_ATOL * (TWENTY_LR0 / 1e-3) * g1
    print("device   :", " ".join("%.6f" % x for x in losses))
    print("float64  :", " ".join("%.6f" % x for x in l64))
    print("step 20: device %.7f, float64 checker %.7f, difference %.3e; sum |gradient| %.3f, margin %.3e"
          % (losses[-1], l64[-1], abs(losses[-1] - l64[-1]), g1, margin))
    assert np.isfinite(losses).all() and losses[-1] < losses[0] and l64[-1] < l64[0], (losses, l64)
    assert abs(losses[-1] - l64[-1]) <= margin, (losses[-1], l64[-1], margin)
    t.save(str(tmp_path))
    trained = t.variables()
    nxt = t.step(*batch)
    t2 = TacotronTrainer(Tacotron(t.model._hparams, num_speakers=h.speakers), randomly_initialized=False, training=True, seed=STEP_SEED)
    assert t2.restore(str(tmp_path)) == TWENTY_STEPS
    same_outputs(trained, t2.variables(), "restored variables")
    assert t2.step(*batch) == nxt
    same_outputs(t.variables(), t2.variables(), "the step after the restore")


def test_training_false_is_the_evaluation_graph_step():
    """TacotronTrainer(training=False) and the constructor's defaults are one step, bit for bit (the recorded digests of the parent's steps
    are profiles/tacotron_train_identity.txt, re-taken by scripts/tacotron_train_identity.py)"""
    from twvk_amd.tacotron_train import TacotronTrainer
    h = step_case(sorted(TWENTY_CASES)[0])
    t, batch = _trainer(h, 1e-3, 1, training=False)
    from twvk_amd.tacotron import Tacotron
    m = Tacotron(t.model._hparams, num_speakers=h.speakers)
    m.load_weights(h.w)
    t0 = TacotronTrainer(m)
    assert t.step(*batch) == t0.step(*batch)
    same_outputs(t.variables(), t0.variables(), "training=False")
    for k, v in t.variables().items():
        if k.endswith("batch_normalization"):
            assert first_mismatch(v[2:], h.w[k][2:]) is None, k


def test_a_refused_model_raises_at_the_first_training_mode_step():
    from twvk_amd._lib import TwvError
    from twvk_amd.tacotron import Tacotron, tacotron_specs
    from twvk_amd.tacotron_train import TacotronTrainer
    import torch_attention_ref as AR
    h = step_case(sorted(TWENTY_CASES)[0])
    for kw, speakers, message in ((dict(model_type="simple"), 4, "model_type 'simple'"), (dict(attention_type="bah_norm"), 2, "attention_type")):
        hp = hparams(max_iters=8, **dict(SMALL, **kw))
        m = Tacotron(hp, num_speakers=speakers)
        m.load_weights(AR.random_tensors(tacotron_specs(hp, speakers), seed=3))
        t = TacotronTrainer(m, training=True)
        with pytest.raises(TwvError, match="twv_amd error 2: .*" + message):
            t.step(h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, h.coeff)
        assert t.global_step == 0
