"""-m "not gpu": the host side of the Tacotron decoder gradients -- the checker itself (tests/torch_tacotron_grad_ref.py: the same mel as
the forward restatement bit for bit; autograd through the in-place helpers anchored by central differences), the exported symbols, every
refusal of twv_tacotron_decoder_grad_create / _run / twv_tacotron_mel_loss_grad / twv_tacotron_workspace_view (all before a device is
looked at), the unchanged size of the inference workspace and the view's pieces."""
import ctypes as C
import functools

import numpy as np
import pytest

R_, MAX_ITERS = 5, 8
SMALL = dict(enc_bank_size=4, post_bank_size=3, num_freq=129)
# what twv_tacotron_workspace_bytes gave before the view was added, at the hparams-default dims, for the (batch, t_in) table of
# tests/test_cpu.py::test_tacotron_workspace_is_sized_by_its_carve (taken from a build of the parent commit)
WS_CASES = ((1, 1), (8, 45), (32, 101), (32, 512), (64, 1024))
WS_PARENT = (29493568, 231162176, 925958464, 952893760, 2014576960)


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _model(num_speakers=2, **kw):
    from twvk_amd.tacotron import Tacotron
    return Tacotron(_hp(max_iters=MAX_ITERS, **dict(SMALL, **kw)), num_speakers=num_speakers)


@pytest.fixture(scope="module")
def model():
    return _model()


@functools.lru_cache(maxsize=None)
def _case(N, T, lengths, steps, seed, attention_type="bah_mon_norm"):
    """weights, tokens, targets, the encoder side and the float64 checker pass of a small case (host only)"""
    import torch_attention_ref as AR
    import torch_tacotron_grad_ref as G
    from twvk_amd.tacotron import tacotron_specs
    hp = _hp(max_iters=MAX_ITERS, attention_type=attention_type, **SMALL)
    specs = tacotron_specs(hp, 2)
    w = AR.random_tensors(specs, seed=seed)
    rng = np.random.RandomState(seed + 1)
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    for n, ln in enumerate(lengths):
        tok[n, ln - 1] = 1
        tok[n, ln:] = 0
    spk = (np.arange(N) % 2).astype(np.int32)
    tgt = rng.uniform(-4.0, 4.0, (N, steps * R_, hp.num_mels)).astype(np.float32)
    d_mel = (rng.randn(N, steps * R_, hp.num_mels) / (N * steps * R_ * hp.num_mels)).astype(np.float32)
    dims = AR.Dims(hp, 2)
    memory, init = G.encoder_side(w, dims, tok, lengths, spk)
    return dict(hp=hp, specs=specs, w=w, tok=tok, ln=np.asarray(lengths, np.int32), spk=spk, tgt=tgt, d_mel=d_mel, dims=dims, memory=memory,
                init=init, names=G.decoder_names(specs))


def test_checker_mel_is_the_forward_restatement_bit_for_bit():
    import torch_tacotron_grad_ref as G
    import torch_tacotron_targets_ref as TR
    for at in ("bah_mon_norm", "bah_mon"):
        c = _case(3, 19, (19, 12, 7), 4, 21, at)
        ref = TR.forward_targets(c["w"], c["dims"], c["tok"], c["ln"], c["spk"], at, c["tgt"], 4 * R_, True)[0]
        mel, grads, _ = G.decoder_vjp(c["w"], c["names"], c["dims"], c["memory"], c["init"], c["ln"], at, c["tgt"], c["d_mel"])
        assert mel.dtype == np.float64 and np.array_equal(mel, ref), at
        assert set(grads) == set(c["names"]) | {"d_memory", "d_init"}
        assert all(np.isfinite(g).all() and g.shape == np.asarray(c["w"][k]).shape for k, g in grads.items() if k in c["w"])
        # the gradient does not flow past a length
        for n, ln in enumerate(c["ln"]):
            assert not grads["d_memory"][n, ln:].any() and grads["d_memory"][n, :ln].any()


def test_checker_gradient_agrees_with_central_differences():
    """float64, eps = 1e-6, three random directions over all leaves at once: (f(x + eps d) - f(x - eps d)) / (2 eps) against g . d, relative
    1e-6 (f = <mel, d_mel>; the truncation error of the central difference is O(eps^2) and its rounding error ~1e-16 / eps = 1e-10 of |f|)."""
    import torch_tacotron_grad_ref as G
    c = _case(2, 11, (11, 6), 3, 31)
    at, eps = "bah_mon_norm", 1e-6
    d_mel = c["d_mel"].astype(np.float64) * 1e3
    _, g, _ = G.decoder_vjp(c["w"], c["names"], c["dims"], c["memory"], c["init"], c["ln"], at, c["tgt"], d_mel)
    base = {k: np.asarray(c["w"][k], np.float64) for k in c["names"]}

    def f(sign, dirs):
        w = {k: base[k] + sign * eps * dirs[k] for k in c["names"]}
        mel = G.decoder_vjp(w, c["names"], c["dims"], c["memory"] + sign * eps * dirs["d_memory"], c["init"] + sign * eps * dirs["d_init"],
                            c["ln"], at, c["tgt"])[0]
        return float((mel * d_mel).sum())
    rng = np.random.RandomState(5)
    for _ in range(3):
        dirs = {k: rng.randn(*np.shape(base[k])) for k in c["names"]}
        dirs["d_memory"] = rng.randn(*c["memory"].shape) * (np.arange(c["memory"].shape[1])[None, :, None] < c["ln"][:, None, None])
        dirs["d_init"] = rng.randn(*c["init"].shape)
        fd = (f(+1, dirs) - f(-1, dirs)) / (2 * eps)
        gd = sum(float((g[k] * dirs[k]).sum()) for k in dirs)
        print("central difference %.12e, g . d %.12e, relative %.2e" % (fd, gd, abs(fd - gd) / abs(gd)))
        assert abs(fd - gd) <= 1e-6 * abs(gd), (fd, gd)


def test_float32_yardstick_is_close_to_float64():
    import torch
    import torch_tacotron_grad_ref as G
    c = _case(3, 19, (19, 12, 7), 4, 21)
    a = (c["w"], c["names"], c["dims"], c["memory"], c["init"], c["ln"], "bah_mon_norm", c["tgt"], c["d_mel"])
    m64, g64, r64 = G.decoder_vjp(*a)
    m32, g32, _ = G.decoder_vjp(*a, dtype=torch.float32)
    assert m32.dtype == np.float32 and all(v.dtype == np.float32 for v in g32.values())
    worst = max(float(np.abs(g32[k] - g64[k]).max()) / float(np.abs(g64[k]).max()) for k in g64)
    assert 0.0 < worst < 1e-4, worst
    assert r64["min_one_minus_p"] > np.finfo(np.float32).tiny and r64["cumprod_margin"] > 1e-3


NEW_SYMBOLS = ("twv_tacotron_workspace_view", "twv_tacotron_decoder_grad_create", "twv_tacotron_decoder_grad_destroy",
               "twv_tacotron_decoder_grad_workspace_bytes", "twv_tacotron_decoder_grad_route", "twv_tacotron_decoder_grad_run",
               "twv_tacotron_decoder_grad_set_timing", "twv_tacotron_decoder_grad_phase_ms", "twv_tacotron_mel_loss_grad")


def test_phase_times_need_a_timed_run(model):
    from twvk_amd import _lib
    g = _create(model)
    try:
        ms = (C.c_double * 3)()
        _lib.check(model._L.twv_tacotron_decoder_grad_set_timing(g, 1))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: no run with timing on"):
            _lib.check(model._L.twv_tacotron_decoder_grad_phase_ms(g, ms))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(model._L.twv_tacotron_decoder_grad_phase_ms(g, None))
    finally:
        model._L.twv_tacotron_decoder_grad_destroy(g)


def test_symbols_are_exported_and_declared():
    import os
    import subprocess
    from twvk_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    L = _lib.lib()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in header and (" T " + name + "\n") in nm, name
    assert "tg_forward_kernel" in nm and "tg_backward_kernel" in nm, "the gfx950 gradient kernels must be in the library"


def _create(m, batch=3, t_in=19, steps=4, h="model", out=True):
    from twvk_amd import _lib
    g = C.c_void_p()
    _lib.check(m._L.twv_tacotron_decoder_grad_create(m._h if h == "model" else None, batch, t_in, steps, C.byref(g) if out else None))
    return g


@pytest.mark.parametrize("kw, message", [
    (dict(h=None), "null argument"), (dict(out=False), "null argument"),
    (dict(steps=0), "1 <= steps <= max_iters"), (dict(steps=MAX_ITERS + 1), "1 <= steps <= max_iters"),
    (dict(batch=0), "batch >= 1"), (dict(t_in=0), "1 <= t_in <= 1024"), (dict(t_in=1025), "1 <= t_in <= 1024"),
])
def test_create_refuses_invalid_arguments(model, kw, message):
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 1: .*" + message):
        _create(model, **kw)


@pytest.mark.parametrize("kw, speakers", [(dict(attention_type=t), 2) for t in ("bah_norm", "bah", "luong", "luong_scaled", "loc_sen")]
                         + [(dict(model_type="simple"), 4)])
def test_create_refuses_what_is_not_built(kw, speakers):
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 2: .*built for attention_type 'bah_mon_norm' and 'bah_mon', single-speaker and 'deepvoice'"):
        _create(_model(num_speakers=speakers, **kw))


@pytest.mark.parametrize("kw, speakers", [({}, 2), (dict(attention_type="bah_mon"), 2), ({}, 1), (dict(dec_layer_num=1), 2),
                                          (dict(speaker_embedding_size=1), 2)])
def test_create_accepts_and_labels_its_route(kw, speakers):
    m = _model(num_speakers=speakers, **kw)
    g = _create(m, 3, 19, 4)
    try:
        route = dict(kv.split("=", 1) for kv in m._L.twv_tacotron_decoder_grad_route(g).decode().split())
        assert route["kernel"] == "tg_bptt" and route["workgroups_per_utterance"] == "1"
        assert route["attention"] == kw.get("attention_type", "bah_mon_norm") and route["layers"] == str(kw.get("dec_layer_num", 2))
        assert int(route["lds_forward"]) <= 160 * 1024 and int(route["lds_backward"]) <= 160 * 1024
        ws = m._L.twv_tacotron_decoder_grad_workspace_bytes(g)
        g2 = _create(m, 3, 19, 8)
        assert m._L.twv_tacotron_decoder_grad_workspace_bytes(g2) > ws > 0
        m._L.twv_tacotron_decoder_grad_destroy(g2)
    finally:
        m._L.twv_tacotron_decoder_grad_destroy(g)


RUN_ARGS = ("g", "blob", "memory", "decoder_init", "lengths", "mel_targets", "d_mel", "mask1", "mask2", "workspace", "status", "stream",
            "mel_out", "grad_blob", "d_memory", "d_init")


@pytest.mark.parametrize("null", [a for a in RUN_ARGS if a not in ("mask1", "mask2", "stream")])
def test_run_refuses_null_arguments(model, null):
    from twvk_amd import _lib
    g = _create(model)
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = [None if n in (null, "mask1", "mask2", "stream") else (g if n == "g" else p) for n in RUN_ARGS]
    try:
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(model._L.twv_tacotron_decoder_grad_run(*a))
    finally:
        model._L.twv_tacotron_decoder_grad_destroy(g)


@pytest.mark.parametrize("null", ["mel", "mel_targets", "coeff", "d_mel"])
def test_mel_loss_grad_refuses_null_arguments(model, null):
    from twvk_amd import _lib
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = {n: (None if n == null else p) for n in ("mel", "mel_targets", "coeff", "d_mel")}
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
        _lib.check(model._L.twv_tacotron_mel_loss_grad(a["mel"], a["mel_targets"], a["coeff"], 3, 25, 80, a["d_mel"], None))
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: batch, t_out and num_mels"):
        _lib.check(model._L.twv_tacotron_mel_loss_grad(p, p, p, 3, 0, 80, p, None))


def test_python_methods_refuse_without_a_teacher_forced_pass(model):
    with pytest.raises(ValueError, match="teacher_forced=True"):
        model.mel_loss_cotangent()
    with pytest.raises(ValueError, match="teacher_forced=True"):
        model.decoder_grad(np.zeros((3, 25, 80), np.float32))


def _view(m, batch, t_in, which):
    from twvk_amd import _lib
    off, n = C.c_longlong(-1), C.c_longlong(-1)
    _lib.check(m._L.twv_tacotron_workspace_view(m._h, batch, t_in, which.encode() if which is not None else None, C.byref(off), C.byref(n)))
    return off.value, n.value


def test_workspace_bytes_are_unchanged_and_the_view_lies_inside():
    import twvk_amd
    from twvk_amd.tacotron import Tacotron
    from twvk_amd._lib import TwvError
    m = Tacotron(twvk_amd.default_hparams(), num_speakers=2)
    got = tuple(int(m._L.twv_tacotron_workspace_bytes(m._h, n, t)) for n, t in WS_CASES)
    assert got == WS_PARENT, got
    hp = m._hparams
    for n, t in WS_CASES:
        total = m._L.twv_tacotron_workspace_bytes(m._h, n, t) // 4
        pieces = sorted(_view(m, n, t, which) for which in ("memory", "keys", "decoder_init"))
        want = {"memory": n * t * 2 * hp.enc_rnn_size, "keys": n * t * hp.attention_size,
                "decoder_init": n * (hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size)}
        assert {w: _view(m, n, t, w)[1] for w in want} == want
        assert pieces[0][0] >= 0 and pieces[-1][0] + pieces[-1][1] <= total
        for (o0, n0), (o1, _) in zip(pieces, pieces[1:]):
            assert o0 + n0 <= o1 and o0 % 4 == 0 and o1 % 4 == 0, (n, t, pieces)
    for bad in ((0, 5, "memory"), (2, 0, "keys"), (2, 1025, "keys"), (2, 5, "values"), (2, 5, None)):
        with pytest.raises(TwvError, match="twv_amd error 1: "):
            _view(m, *bad)
