"""-m "not gpu": the host side of the Tacotron training-mode graph -- the checker itself (tests/torch_tacotron_trainmode_ref.py:
its batch norm against the plain definition and against the inference restatement at the batch's own statistics, autograd anchored by
central differences, the zero gradient of a bias in front of a batch norm), the margin and yardstick conditions of every case of the GPU
tables, the moving-average and dropout-mask restatements' known answers, the exported symbols and every refusal of the new entries that
comes before a device is looked at."""
import ctypes as C

import numpy as np
import pytest

from tacotron_trainmode_cases import (CASES, MARGIN, SMALL, STEP_CASES, TWENTY_CASES, TWENTY_STEPS, ZERO_GRADIENTS, checker_trajectory, hparams, host_case, step_case,
                                      step_conditions)

MAX_ITERS = 8


@pytest.fixture(scope="module")
def model():
    from twvk_amd.tacotron import Tacotron
    return Tacotron(hparams(max_iters=MAX_ITERS, **SMALL), num_speakers=2)


# ---------------------------------------------------------------- the checker
def test_batch_form_is_the_definition_and_the_inference_form_at_its_own_statistics():
    import torch
    import torch_tacotron_cbhg_grad_ref as CG
    import torch_tacotron_ref as R
    import torch_tacotron_trainmode_ref as TM
    h = host_case("A-masked-tails")
    rng = np.random.RandomState(2)
    x = torch.as_tensor(rng.randn(3, 7, 5) * 2.0 + 1.0)
    bn = torch.as_tensor(np.stack([rng.uniform(0.5, 1.5, 5), rng.randn(5), rng.randn(5), rng.uniform(0.5, 2.0, 5)]))
    stats = []
    with TM.batch_norm_training(stats):
        y = R._batch_norm_inference(x, bn)
    flat = x.reshape(-1, 5).numpy()
    mean, var = flat.mean(0), flat.var(0)                   # numpy's var is the biased one
    assert np.allclose(stats[0][0], mean, rtol=1e-14) and np.allclose(stats[0][1], var, rtol=1e-13)
    want = (x.numpy() - mean) / np.sqrt(var + 1e-3) * bn[0].numpy() + bn[1].numpy()
    assert float(np.abs(y.numpy() - want).max()) <= 1e-14 * float(np.abs(want).max())
    assert R._batch_norm_inference(x, bn) is not None and len(stats) == 1           # (the inference form is back after the block)
    # the whole encoder / post net: the inference restatement on weights whose moving statistics are the batch's gives the same outputs
    for which, run, plain, names in (("encoder", h.encoder_checker, lambda w: CG.encoder_vjp(w, h.enc_names, h.dims, h.tok, h.ln, h.bh, h.init)[0], h.enc_names),
                                     ("post", h.postnet_checker, lambda w: CG.postnet_vjp(w, h.post_names, h.dims, h.mel)[0], h.post_names)):
        out, _, _, st = run("float64")
        w = dict(h.w)
        for k, s in st.items():
            w[k] = np.concatenate([np.asarray(h.w[k], np.float64)[:2], s])
        assert len(st) == sum(1 for k in names if k.endswith("batch_normalization")) > 0
        assert float(np.abs(plain(w) - out).max()) <= 1e-12 * float(np.abs(out).max()), which


def test_checker_gradients_agree_with_central_differences():
    """float64, three random directions over all leaves at once, as tests/test_tacotron_cbhg_grad_cpu.py holds the evaluation graph's
    checker: (f(x + eps d) - f(x - eps d)) / (2 eps) against g . d, relative 1e-6.  eps = 1e-8 here: a unit direction over every leaf moves
    a pre-activation by about ten times eps, and this table's smallest relu margin is 2e-6 -- at eps = 1e-6 the two evaluations straddle
    a kink (the post net's difference is then 7e-4 off).  The rounding of f (about 1e-12 of it) leaves 1e-8 at this eps."""
    import torch_tacotron_trainmode_ref as TM
    h = host_case("A-masked-tails")
    eps, rng = 1e-8, np.random.RandomState(5)
    d_mem, d_lin = h.d_memory.astype(np.float64) * 1e3, h.d_linear.astype(np.float64) * 1e3
    ge = TM.encoder_vjp(h.w, h.enc_names, h.dims, h.tok, h.ln, h.bh, h.init, d_mem)[1]
    gp = TM.postnet_vjp(h.w, h.post_names, h.dims, h.mel, d_lin)[1]

    def full(name, g):
        return np.concatenate([g, np.zeros_like(g)]) if name.endswith("batch_normalization") else g
    for _ in range(3):
        base = {k: np.asarray(h.w[k], np.float64) for k in h.enc_names + h.post_names}
        # (the moving statistics take directions too: the training-mode output does not depend on them)
        dirs = {k: rng.randn(*base[k].shape) for k in base}
        dirs["embedding"][0] = 0.0
        db, di, dm = rng.randn(*h.bh.shape), rng.randn(*h.init.shape), rng.randn(*h.mel.shape)

        def fe(s):
            w = {k: base[k] + s * eps * dirs[k] for k in h.enc_names}
            return float((TM.encoder_vjp(w, h.enc_names, h.dims, h.tok, h.ln, h.bh + s * eps * db, h.init + s * eps * di)[0] * d_mem).sum())

        def fp(s):
            w = {k: base[k] + s * eps * dirs[k] for k in h.post_names}
            return float((TM.postnet_vjp(w, h.post_names, h.dims, h.mel + s * eps * dm)[0] * d_lin).sum())
        for label, f, gd in (("encoder", fe, sum(float((full(k, ge[k]) * dirs[k]).sum()) for k in h.enc_names)
                              + float((ge["d_before_highway"] * db).sum()) + float((ge["d_rnn_init"] * di).sum())),
                             ("post net", fp, sum(float((full(k, gp[k]) * dirs[k]).sum()) for k in h.post_names) + float((gp["d_mel"] * dm).sum()))):
            fd = (f(+1) - f(-1)) / (2 * eps)
            print("%s: central difference %.12e, g . d %.12e, relative %.2e" % (label, fd, gd, abs(fd - gd) / abs(gd)))
            assert abs(fd - gd) <= 1e-6 * abs(gd), (label, fd, gd)


def test_a_bias_in_front_of_a_batch_norm_has_no_gradient():
    """proj_2 has no relu between its convolution and its batch norm, so its bias is a constant the batch norm removes: float64 autograd
    leaves rounding noise of the order 1e-17, float32 of the order 1e-8, where the same convolution's kernel has a gradient of 0.01 .. 0.1"""
    for name in sorted(CASES):
        h = host_case(name)
        for run, bias in ((h.encoder_checker, ZERO_GRADIENTS[0]), (h.postnet_checker, ZERO_GRADIENTS[1])):
            g64, g32 = run("float64")[1], run("float32")[1]
            kernel = float(np.abs(g64[bias[:-4] + "kernel"]).max())
            print("%s %s: float64 %.3e, float32 %.3e, kernel %.3e" % (name, bias, float(np.abs(g64[bias]).max()), float(np.abs(g32[bias]).max()), kernel))
            assert float(np.abs(g64[bias]).max()) <= 1e-12 * max(kernel, 1e-30) or name == "K-one-row"
            if name == "K-one-row":
                assert not g64[bias].any() and not g64[bias[:-4] + "kernel"].any()


# ---------------------------------------------------------------- the conditions of the GPU tables
@pytest.mark.parametrize("name", sorted(CASES))
def test_margin_condition_of_the_gpu_table(name):
    same, relu_margin, pool_gap = host_case(name).margins()
    print("%s: relu margin %.3e, pool gap %.3e" % (name, relu_margin, pool_gap))
    assert same and relu_margin > MARGIN and pool_gap > MARGIN, (name, same, relu_margin, pool_gap)


def test_table_covers_the_shapes_it_is_for():
    from tacotron_cbhg_grad_cases import CASES as OLD
    N, T, _, TO = CASES["J-chunks"][:4]
    assert 128 < N * T < 256 and 256 < N * TO < 384 and (N * T) % 128 and (N * TO) % 128 and (N * TO) % 4
    assert CASES["K-one-row"][:4] == (1, 1, (1,), 1)
    assert CASES["E-single-speaker"][4] == 1 and CASES["F-speaker-tables"][5] == dict(speaker_embedding_size=1) and CASES["I-dropout-masks"][6]
    assert CASES["H-odd-channels"][5]["post_bank_size"] == 4 and CASES["H-odd-channels"][5]["enc_bank_channel_size"] == 30
    assert CASES["G-bank-one-depth-one"][5]["enc_bank_size"] == 1
    assert not {row[-1] for row in CASES.values()} & {row[-1] for row in OLD.values()}          # seeds of this table's own


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_conditions_of_the_step_cases(name):
    ok, fig = step_conditions(step_case(name))
    print(name, fig)
    assert ok, fig


def test_checker_trajectory_falls():
    l64, g1 = checker_trajectory(sorted(TWENTY_CASES)[0])
    print("float64 checker, training mode:", " ".join("%.6f" % x for x in l64), "; sum |gradient| at step 20: %.3f" % g1)
    assert len(l64) == TWENTY_STEPS and np.isfinite(l64).all() and l64[-1] < l64[0] and 0.0 < g1 < float("inf"), l64


# ---------------------------------------------------------------- restatements: known answers
def test_moving_average_known_answers():
    import torch_tacotron_trainmode_ref as TM
    from twvk_amd.tacotron import BN_MOMENTUM, moving_average_update
    assert BN_MOMENTUM == TM.MOMENTUM == 0.99
    assert TM.moving_average(1.0, 0.0) == pytest.approx(0.99, rel=1e-15) and TM.moving_average(0.0, 1.0) == pytest.approx(0.01, rel=1e-13)
    assert TM.moving_average(2.5, 2.5) == 2.5
    decay = np.float32(1.0 - 0.99)
    assert decay == np.float32(0.01) and float(decay) == 0.009999999776482582
    m, b = np.float32([1.0, 0.0, 2.5, -3.0, 1e-3]), np.float32([0.0, 1.0, 2.5, 5.0, 1.0])
    got = moving_average_update(m, b)
    assert got.dtype == np.float32
    # each operation rounded to float32, spelled out
    want = [np.float32(mi - np.float32(np.float32(mi - bi) * decay)) for mi, bi in zip(m, b)]
    assert got.tolist() == [float(v) for v in want]
    assert got[0] == np.float32(0.99) and got[1] == np.float32(0.01) and got[2] == np.float32(2.5)
    assert float(np.abs(got - TM.moving_average(m, b)).max()) <= 4 * 2.0 ** -24 * 5.0
    # a hundred updates toward a constant: 1 - 0.99^100 of the way
    v = np.float32([0.0])
    for _ in range(100):
        v = moving_average_update(v, np.float32([1.0]))
    assert float(v[0]) == pytest.approx(1.0 - 0.99 ** 100, rel=1e-5)


def test_dropout_mask_restatement_known_answers():
    from twvk_amd.tacotron import DROPOUT_SITES, dropout_mask_numpy
    M64 = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)
    # the finaliser is splitmix64's: its first outputs from state 0 are the published 0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4
    G = 0x9E3779B97F4A7C15
    assert mix(G) == 0xE220A8397B1DCDAF and mix((2 * G) & M64) == 0x6E789E6AA1B965F4
    for seed, step, site, rate in ((0, 0, 0, 0.5), (7, 3, 2, 0.5), (2 ** 63 + 5, 1000000, 3, 0.25), (11, 0, 1, 0.0)):
        key = mix((seed + G * (4 * step + site)) & M64)
        want = []
        for i in range(300):
            u = np.float32(mix((key + G * (i + 1)) & M64) >> 40) * np.float32(2.0 ** -24)
            want.append(np.float32(1.0 / (1.0 - rate)) if u >= np.float32(rate) else np.float32(0.0))
        got = dropout_mask_numpy(300, seed, step, site, rate)
        assert got.dtype == np.float32 and got.tolist() == [float(v) for v in want], (seed, step, site)
    assert set(dropout_mask_numpy(4096, 1, 0, 0).tolist()) == {0.0, 2.0}
    assert dropout_mask_numpy(4096, 1, 0, 0, 0.0).tolist() == [1.0] * 4096
    assert sorted(DROPOUT_SITES.values()) == [0, 1, 2, 3]
    a = dropout_mask_numpy(4096, 1, 0, 0)
    for other in (dropout_mask_numpy(4096, 1, 0, 1), dropout_mask_numpy(4096, 1, 1, 0), dropout_mask_numpy(4096, 2, 0, 0)):
        assert abs(float((a != other).mean()) - 0.5) <= 5.0 * np.sqrt(0.25 / 4096)
    # an element does not depend on how many are drawn
    assert np.array_equal(dropout_mask_numpy(100, 1, 0, 0), a[:100])


# ---------------------------------------------------------------- the C surface
NEW_SYMBOLS = ("twv_tacotron_decoder_grad_forward", "twv_tacotron_decoder_grad_backward", "twv_tacotron_encoder_grad_forward",
               "twv_tacotron_encoder_grad_backward", "twv_tacotron_postnet_grad_forward", "twv_tacotron_postnet_grad_backward",
               "twv_tacotron_cbhg_grad_set_mode", "twv_tacotron_cbhg_grad_batch_stats_floats", "twv_tacotron_cbhg_grad_batch_stats",
               "twv_tacotron_grad_convert_batch", "twv_tacotron_moving_update", "twv_dropout_mask")


def test_symbols_are_exported_and_declared():
    import os
    import subprocess
    from twvk_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    L = _lib.lib()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in header and (" T " + name + "\n") in nm, name
    assert "#define TWV_BN_INFERENCE 0" in header and "#define TWV_BN_BATCH 1" in header
    for kernel in ("cg_stats_kernel", "cg_stats_finish_kernel", "cg_bn_apply_kernel", "cg_bn_batch_sums_kernel", "cg_bn_batch_finish_kernel",
                   "cg_bn_batch_bwd_kernel"):          # (the training file's kernels have internal linkage and no dynamic symbol)
        assert kernel in nm, "the gfx950 kernel %s must be in the library" % kernel


def _cbhg(m, which=0, batch=3, t=19):
    from twvk_amd import _lib
    g = C.c_void_p()
    _lib.check(m._L.twv_tacotron_cbhg_grad_create(m._h, which, batch, t, C.byref(g)))
    return g


def _dummy():
    buf = (C.c_float * 16)()
    return buf, C.cast(buf, C.c_void_p)


def test_a_backward_needs_its_forward_and_its_own_kind_of_handle(model):
    from twvk_amd import _lib
    L = model._L
    keep, p = _dummy()
    ge, gp = _cbhg(model), _cbhg(model, 1, 3, 40)
    gd = C.c_void_p()
    _lib.check(L.twv_tacotron_decoder_grad_create(model._h, 3, 19, 8, C.byref(gd)))
    try:
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: backward: no forward has been made on this handle .twv_tacotron_encoder_grad_forward"):
            _lib.check(L.twv_tacotron_encoder_grad_backward(ge, p, p, p, p, p, p, None, p, None, None))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: backward: no forward has been made on this handle .twv_tacotron_postnet_grad_forward"):
            _lib.check(L.twv_tacotron_postnet_grad_backward(gp, p, p, p, p, p, None, p, p))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: backward: no forward has been made on this handle .twv_tacotron_decoder_grad_forward"):
            _lib.check(L.twv_tacotron_decoder_grad_backward(gd, p, p, p, p, p, p, p, None, p, p, p))
        for call, other in ((lambda g: L.twv_tacotron_encoder_grad_forward(g, p, p, p, None, None, None, None, p, p, None, p), gp),
                            (lambda g: L.twv_tacotron_encoder_grad_backward(g, p, p, p, p, p, p, None, p, None, None), gp)):
            with pytest.raises(_lib.TwvError, match="twv_amd error 1: the handle was created for the post net"):
                _lib.check(call(other))
        for call in (lambda g: L.twv_tacotron_postnet_grad_forward(g, p, p, p, p, None, p), lambda g: L.twv_tacotron_postnet_grad_backward(g, p, p, p, p, p, None, p, p)):
            with pytest.raises(_lib.TwvError, match="twv_amd error 1: the handle was created for the encoder"):
                _lib.check(call(ge))
        # null arguments, each half
        for call in (lambda: L.twv_tacotron_encoder_grad_forward(ge, p, p, p, None, None, None, None, p, p, None, None),
                     lambda: L.twv_tacotron_encoder_grad_backward(ge, p, p, p, None, p, p, None, p, None, None),
                     lambda: L.twv_tacotron_postnet_grad_forward(gp, p, None, p, p, None, p),
                     lambda: L.twv_tacotron_postnet_grad_backward(gp, p, p, p, p, p, None, None, p),
                     lambda: L.twv_tacotron_decoder_grad_forward(gd, p, p, p, p, None, None, None, p, p, None, p),
                     lambda: L.twv_tacotron_decoder_grad_backward(gd, p, p, p, p, p, p, p, None, p, p, None),
                     lambda: L.twv_tacotron_encoder_grad_forward(None, p, p, p, None, None, None, None, p, p, None, p)):
            with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
                _lib.check(call())
    finally:
        L.twv_tacotron_cbhg_grad_destroy(ge)
        L.twv_tacotron_cbhg_grad_destroy(gp)
        L.twv_tacotron_decoder_grad_destroy(gd)
    assert keep is not None


def test_mode_statistics_update_and_mask_refusals(model):
    from twvk_amd import _lib
    L = model._L
    keep, p = _dummy()
    g = _cbhg(model)
    try:
        for mode in (-1, 2):
            with pytest.raises(_lib.TwvError, match="twv_amd error 1: mode must be TWV_BN_INFERENCE"):
                _lib.check(L.twv_tacotron_cbhg_grad_set_mode(g, mode, p))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: batch mode needs the training vector"):
            _lib.check(L.twv_tacotron_cbhg_grad_set_mode(g, 1, None))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(L.twv_tacotron_cbhg_grad_set_mode(None, 0, None))
        _lib.check(L.twv_tacotron_cbhg_grad_set_mode(g, 0, None))          # inference: no vector, nothing allocated
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: batch statistics: no forward in batch mode"):
            _lib.check(L.twv_tacotron_cbhg_grad_batch_stats(g, p, None))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(L.twv_tacotron_cbhg_grad_batch_stats(g, None, None))
        hp = model._hparams
        assert L.twv_tacotron_cbhg_grad_batch_stats_floats(g) == 2 * (hp.enc_bank_size * hp.enc_bank_channel_size + sum(hp.enc_proj_sizes))
        assert L.twv_tacotron_cbhg_grad_batch_stats_floats(None) == 0
    finally:
        L.twv_tacotron_cbhg_grad_destroy(g)
    for args in ((None, p, p, p), (model._h, None, p, p), (model._h, p, None, p), (model._h, p, p, None)):
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(L.twv_tacotron_moving_update(*(args + (0.99, None))))
    for momentum in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: momentum must lie in"):
            _lib.check(L.twv_tacotron_moving_update(model._h, p, p, p, momentum, None))
    for args in ((None, p, p), (model._h, None, p), (model._h, p, None)):
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(L.twv_tacotron_grad_convert_batch(*(args + (None,))))
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
        _lib.check(L.twv_dropout_mask(None, 16, 0, 0, 0, 0.5, None))
    for n, step, site, rate, message in ((0, 0, 0, 0.5, "n >= 1"), (16, -1, 0, 0.5, "step >= 0"), (16, 0, 4, 0.5, "site 0 .. 3"), (16, 0, -1, 0.5, "site 0 .. 3"),
                                         (16, 0, 0, 1.0, "rate must lie in"), (16, 0, 0, -0.1, "rate must lie in")):
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: .*" + message):
            _lib.check(L.twv_dropout_mask(p, n, 0, step, site, rate, None))
    assert keep is not None


def test_python_methods_refuse_before_the_device(model):
    for call in (lambda: model.encoder_grad_forward(mode="batch"), lambda: model.decoder_grad_forward(),
                 lambda: model.encoder_grad(np.zeros((3, 19, 256), np.float32), mode="batch"), lambda: model.postnet_grad(np.zeros((3, 25, 129), np.float32), mode="batch")):
        with pytest.raises(ValueError, match="teacher_forced=True"):
            call()
    for call, message in ((lambda: model.encoder_grad_backward(np.zeros((3, 19, 256), np.float32)), "needs encoder_grad_forward first"),
                          (lambda: model.postnet_grad_backward(np.zeros((3, 25, 129), np.float32)), "needs postnet_grad_forward first"),
                          (lambda: model.decoder_grad_backward(np.zeros((3, 25, 80), np.float32)), "needs decoder_grad_forward first"),
                          (lambda: model.batch_statistics("encoder"), "needs a batch-mode pass first")):
        with pytest.raises(ValueError, match=message):
            call()
    with pytest.raises(KeyError):
        model.batch_statistics("decoder")
    from twvk_amd.tacotron_train import TacotronTrainer
    t = TacotronTrainer(model, training=True, seed=5)
    assert t.training and t.seed == 5 and not TacotronTrainer(model).training
