"""-m "not gpu": the host side of the decoder gradients at the softmax attention types and loc_sen -- the new export
(twv_tacotron_decoder_grad_create_any), what it accepts, labels and refuses (all before a device is looked at), Tacotron.attention_gradients,
the checker anchored by central differences for each new kind, and the case table's conditions on the smallest case of each kind."""
import ctypes as C

import numpy as np
import pytest

from tacotron_grad_cases import R_, SMALL, hparams

MAX_ITERS = 8
TYPES = ("bah_mon_norm", "bah_mon", "bah_norm", "bah", "luong", "luong_scaled", "loc_sen")


def _model(num_speakers=2, **kw):
    from twvk_amd.tacotron import Tacotron
    return Tacotron(hparams(max_iters=MAX_ITERS, **dict(SMALL, **kw)), num_speakers=num_speakers)


def _create(m, batch=3, t_in=19, steps=4, entry="twv_tacotron_decoder_grad_create_any"):
    from twvk_amd import _lib
    g = C.c_void_p()
    _lib.check(getattr(m._L, entry)(m._h, batch, t_in, steps, C.byref(g)))
    return g


def _route(m, g):
    return dict(kv.split("=", 1) for kv in m._L.twv_tacotron_decoder_grad_route(g).decode().split())


def test_the_symbol_is_exported_declared_and_bound():
    import os
    import subprocess
    from twvk_amd import _lib
    name = "twv_tacotron_decoder_grad_create_any"
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    L = _lib.lib()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert name in _lib.EXPORTS and name + "(" in header and (" T " + name + "\n") in nm
    assert getattr(L, name).argtypes == L.twv_tacotron_decoder_grad_create.argtypes
    assert "tg_forward_kernel" in nm and "tg_backward_kernel" in nm and "tg_loc_derive_kernel" in nm


@pytest.mark.parametrize("at", TYPES)
def test_create_any_accepts_every_type_and_labels_it(at):
    m = _model(attention_type=at)
    g, g8 = _create(m, 3, 19, 4), _create(m, 3, 19, 8)
    try:
        route = _route(m, g)
        assert route["kernel"] == "tg_bptt" and route["attention"] == at and route["workgroups_per_utterance"] == "1" and route["layers"] == "2"
        assert int(route["lds_forward"]) <= 160 * 1024 and int(route["lds_backward"]) <= 160 * 1024
        ws, ws8 = (m._L.twv_tacotron_decoder_grad_workspace_bytes(x) for x in (g, g8))
        assert ws8 > ws > 0                                     # the tape grows with the steps
        if at in ("bah_mon_norm", "bah_mon"):                   # the handle _create makes: same workspace, same label
            g0 = _create(m, 3, 19, 4, entry="twv_tacotron_decoder_grad_create")
            assert m._L.twv_tacotron_decoder_grad_workspace_bytes(g0) == ws
            assert m._L.twv_tacotron_decoder_grad_route(g0) == m._L.twv_tacotron_decoder_grad_route(g)
            m._L.twv_tacotron_decoder_grad_destroy(g0)
    finally:
        m._L.twv_tacotron_decoder_grad_destroy(g)
        m._L.twv_tacotron_decoder_grad_destroy(g8)


def test_the_tape_is_carved_by_kind():
    """at one size: Luong has no query-layer pieces, the softmax kinds none of the three monotonic arrays, loc_sen its own on top"""
    ws = {}
    for at in ("bah_mon_norm", "bah_norm", "luong", "loc_sen"):
        m = _model(attention_type=at)
        g = _create(m, 3, 19, 4)
        ws[at] = m._L.twv_tacotron_decoder_grad_workspace_bytes(g)
        m._L.twv_tacotron_decoder_grad_destroy(g)
    rows, T, A = 3 * 4, 19, 256
    take = lambda n: (n + 3) // 4 * 4 * 4          # bytes of a piece: rounded up to four floats
    assert ws["bah_mon_norm"] - ws["bah_norm"] == 3 * take(rows * T)
    assert ws["bah_norm"] - ws["luong"] == 2 * take(rows * A)
    assert ws["loc_sen"] > ws["bah_norm"]


def test_create_any_keeps_the_other_refusals_and_reshape_follows_its_door():
    from twvk_amd import _lib
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 2: .*model_type 'simple': the decoder gradient is built for"):
        _create(_model(num_speakers=4, model_type="simple", attention_type="bah_norm"))
    m = _model(attention_type="loc_sen")
    for kw, message in ((dict(steps=0), "1 <= steps <= max_iters"), (dict(steps=MAX_ITERS + 1), "1 <= steps <= max_iters"), (dict(batch=0), "batch >= 1"),
                        (dict(t_in=1025), "1 <= t_in <= 1024")):
        with pytest.raises(TwvError, match="twv_amd error 1: .*" + message):
            _create(m, **kw)
    with pytest.raises(TwvError, match="twv_amd error 1: null argument"):
        _lib.check(m._L.twv_tacotron_decoder_grad_create_any(None, 3, 19, 4, C.byref(C.c_void_p())))
    g = _create(m, 3, 19, 4)
    try:
        label, ws = m._L.twv_tacotron_decoder_grad_route(g), m._L.twv_tacotron_decoder_grad_workspace_bytes(g)
        with pytest.raises(TwvError, match="twv_amd error 1: .*1 <= t_in <= 1024"):
            _lib.check(m._L.twv_tacotron_decoder_grad_reshape(g, 3, 1025, 4))
        assert (m._L.twv_tacotron_decoder_grad_route(g), m._L.twv_tacotron_decoder_grad_workspace_bytes(g)) == (label, ws)
        _lib.check(m._L.twv_tacotron_decoder_grad_reshape(g, 5, 40, 8))          # accepted: the handle came through _create_any
        g2 = _create(m, 5, 40, 8)
        assert m._L.twv_tacotron_decoder_grad_route(g) == m._L.twv_tacotron_decoder_grad_route(g2)
        assert m._L.twv_tacotron_decoder_grad_workspace_bytes(g) == m._L.twv_tacotron_decoder_grad_workspace_bytes(g2) > ws
        m._L.twv_tacotron_decoder_grad_destroy(g2)
        # the backward needs a forward at the new sizes, on either kind of handle
        p = C.cast((C.c_float * 16)(), C.c_void_p)
        with pytest.raises(TwvError, match="twv_amd error 1: backward: no forward has been made"):
            _lib.check(m._L.twv_tacotron_decoder_grad_backward(g, p, p, p, p, p, p, p, None, p, p, p))
    finally:
        m._L.twv_tacotron_decoder_grad_destroy(g)


def test_attention_gradients_is_an_opt_in_that_drops_the_cached_handle():
    m = _model(attention_type="luong")
    assert m.attention_gradients == "monotonic"
    for bad in ("all", None, 1, "Any"):
        with pytest.raises(ValueError, match="attention_gradients"):
            m.attention_gradients = bad
    assert m.attention_gradients == "monotonic"
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 2: .*attention_type"):
        m._grad_handle("decoder", (3, 19, 4))                  # the default door: refused before anything is allocated
    assert "decoder" not in getattr(m, "_grad_cache", {})
    m.attention_gradients = "any"
    g = _create(m)
    m.__dict__.setdefault("_grad_cache", {})["decoder"] = ((3, 19, 4), g, None)        # as _grad_handle leaves it
    m.attention_gradients = "any"                                                       # no change: the handle stays
    assert "decoder" in m._grad_cache
    m.attention_gradients = "monotonic"
    assert "decoder" not in m._grad_cache and m.decoder_grad_route() == ""


def test_the_trainer_sets_it_on_the_model_and_train_tacotron_asks_for_any():
    import inspect
    from twvk_amd import train_tacotron
    from twvk_amd.tacotron_train import TacotronTrainer
    assert inspect.signature(TacotronTrainer.__init__).parameters["attention_gradients"].default is None
    m = _model(attention_type="loc_sen")
    TacotronTrainer(m)
    assert m.attention_gradients == "monotonic"              # the model's default, left alone
    TacotronTrainer(m, attention_gradients="any")
    assert m.attention_gradients == "any"
    TacotronTrainer(m)
    assert m.attention_gradients == "any"                    # None leaves what the caller set
    TacotronTrainer(m, attention_gradients="monotonic")
    assert m.attention_gradients == "monotonic"
    with pytest.raises(ValueError, match="attention_gradients"):
        TacotronTrainer(m, attention_gradients="softmax")
    assert 'attention_gradients="any"' in inspect.getsource(train_tacotron)


@pytest.mark.parametrize("at", ["bah_norm", "luong_scaled", "loc_sen"])
def test_checker_gradient_agrees_with_central_differences(at):
    """the anchor tests/test_tacotron_grad_cpu.py has for the monotonic types, for one small case of each new kind: float64, eps = 1e-6,
    three random directions over all leaves at once, (f(x + eps d) - f(x - eps d)) / (2 eps) against g . d, relative 1e-6"""
    import torch_attention_ref as AR
    import torch_tacotron_grad_ref as G
    from tacotron_attention_grad_cases import SHARPENED
    from tacotron_grad_cases import padded_tokens
    from twvk_amd.tacotron import tacotron_specs
    N, T, lengths, steps, seed, eps = 2, 11, (11, 6), 3, 31, 1e-6
    hp = hparams(max_iters=MAX_ITERS, attention_type=at, **SMALL)
    specs = tacotron_specs(hp, 2)
    w = AR.random_tensors(specs, seed=seed)
    sharp = [n for n, _ in specs if n == SHARPENED[at] or n.endswith("/" + SHARPENED[at])][0]
    w[sharp] = w[sharp] * np.float32(6.0)
    rng = np.random.RandomState(seed + 1)
    tok, ln, spk = padded_tokens(rng, N, T, lengths), np.asarray(lengths, np.int32), (np.arange(N) % 2).astype(np.int32)
    tgt = rng.uniform(-4.0, 4.0, (N, steps * R_, hp.num_mels)).astype(np.float32)
    d_mel = rng.randn(N, steps * R_, hp.num_mels) / (N * steps * R_ * hp.num_mels) * 1e3
    dims, names = AR.Dims(hp, 2), G.decoder_names(specs)
    memory, init = G.encoder_side(w, dims, tok, ln, spk)
    _, g, _ = G.decoder_vjp(w, names, dims, memory, init, ln, at, tgt, d_mel)
    base = {k: np.asarray(w[k], np.float64) for k in names}

    def f(sign, dirs):
        ww = {k: base[k] + sign * eps * dirs[k] for k in names}
        mel = G.decoder_vjp(ww, names, dims, memory + sign * eps * dirs["d_memory"], init + sign * eps * dirs["d_init"], ln, at, tgt)[0]
        return float((mel * d_mel).sum())
    rng = np.random.RandomState(5)
    for _ in range(3):
        dirs = {k: rng.randn(*np.shape(base[k])) for k in names}
        dirs["d_memory"] = rng.randn(*memory.shape) * (np.arange(T)[None, :, None] < ln[:, None, None])
        dirs["d_init"] = rng.randn(*init.shape)
        fd = (f(+1, dirs) - f(-1, dirs)) / (2 * eps)
        gd = sum(float((g[k] * dirs[k]).sum()) for k in dirs)
        print("%s: central difference %.12e, g . d %.12e, relative %.2e" % (at, fd, gd, abs(fd - gd) / abs(gd)))
        assert abs(fd - gd) <= 1e-6 * abs(gd), (at, fd, gd)


@pytest.mark.parametrize("name", ["bah_norm-tails", "luong_scaled-tails", "loc_sen-tails", "bah_norm-length-one", "bah-one-step"])
def test_case_table_conditions(name):
    """the three conditions of tests/tacotron_attention_grad_cases.py at the table's seed and factor (every case:
    scripts/tacotron_attention_grad_parity.py --seeds, recorded in profiles/tacotron_attention_grad_parity.txt)"""
    from tacotron_attention_grad_cases import HostCase, conditions_hold
    c = HostCase(name)
    zero, worst, amax = c.conditions()
    print(name, zero, worst, amax)
    assert conditions_hold(c, zero, worst, amax), (zero, worst, amax)
