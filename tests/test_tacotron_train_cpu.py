"""-m "not gpu": the host side of the Tacotron training step.  The checker tests/torch_tacotron_speaker_grad_ref.py is
anchored against central differences; the schedule has known answers; the training vector's layout covers every tensor once; the new C
entries refuse what they document without touching a device; and every whole-model case the device tests use meets the margin conditions
of tests/test_tacotron_cbhg_grad_cpu.py's chain cases, with the speaker tensors among the tensors looked at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tacotron_cbhg_grad_cases import CHAIN_E_T32, MARGIN
from tacotron_train_cases import SPEAKER_CASES, TWENTY_LR0, TWENTY_MODE, TWENTY_STEPS, WHOLE, hparams, SMALL, speaker_case, whole_case, whole_checker

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("twv_tacotron_speaker_grad_scratch_bytes", "twv_tacotron_speaker_grad", "twv_tacotron_train_floats", "twv_tacotron_refold",
                    "twv_tacotron_grad_convert")


def _model(num_speakers=2, **kw):
    from twvk_amd.tacotron import Tacotron
    return Tacotron(hparams(max_iters=8, **dict(SMALL, **kw)), num_speakers=num_speakers)


# ---------------------------------------------------------------- the checker
@pytest.mark.parametrize("name", ["a-three", "b-nine-unnamed-speaker", "d-tables", "f-one-layer"])
def test_speaker_vjp_is_the_derivative_of_speaker_side(name):
    """float64 autograd against central differences of the forward along a random direction of every speaker tensor: 1e-6 relative"""
    import torch_tacotron_cbhg_grad_ref as CG
    import torch_tacotron_speaker_grad_ref as SG
    c = speaker_case(name)
    names = SG.speaker_names(c.w, c.dims)
    assert names == [n for n, _ in c.specs][1:1 + len(names)] and c.specs[1 + len(names)][0] == "prenet/dense_1/kernel"
    g = c.checker("float64")
    # the restated forward is CG.speaker_side's, value for value
    for a, b in zip(SG.speaker_side(c.w, c.dims, c.ids), CG.speaker_side(c.w, c.dims, c.ids)):
        assert np.array_equal(a, b)
    rng = np.random.RandomState(5)
    direction = {k: rng.randn(*np.shape(c.w[k])) for k in names}
    cot = [np.asarray(v, np.float64) for v in c.cot]

    def f(e):
        w = dict(c.w)
        w.update({k: np.asarray(c.w[k], np.float64) + e * direction[k] for k in names})
        return sum(float((o * d).sum()) for o, d in zip(SG.speaker_side(w, c.dims, c.ids), cot))
    e = 1e-5
    fd = (f(e) - f(-e)) / (2 * e)
    an = sum(float((g[k] * direction[k]).sum()) for k in names)
    print("%s: central difference %.12e autograd %.12e" % (name, fd, an))
    assert abs(fd - an) <= 1e-6 * abs(fd), (fd, an)
    for k in names:
        assert g[k].shape == np.shape(c.w[k]) and np.isfinite(g[k]).all(), k
    unnamed = sorted(set(range(c.speakers)) - set(int(i) for i in c.ids))
    for k in (["speaker_embedding"] if "speaker_embedding" in c.w else names):
        assert all(not g[k][s].any() for s in unnamed) and g[k][int(c.ids[0])].any(), k


def test_train_step_checker_known_answers():
    import torch_tacotron_speaker_grad_ref as SG
    var = {"a": np.array([1.0, -2.0]), "bn/batch_normalization": np.arange(8.0).reshape(4, 2)}
    grads = {"a": np.array([3.0, 0.0]), "bn/batch_normalization": np.array([[0.0, 4.0], [0.0, 0.0]])}
    zeros = {k: np.zeros_like(v) for k, v in var.items()}
    nv, nm, nvv, norm, clipped = SG.train_step(var, grads, zeros, zeros, 1, 0.01, 0.9, 0.999)
    assert norm == 5.0 and np.allclose(clipped["a"], [0.6, 0.0]) and np.allclose(clipped["bn/batch_normalization"][0], [0.0, 0.8])
    # the first Adam step moves every variable with a gradient by lr against its sign, and no other
    assert np.allclose(nv["a"], [0.99, -2.0], atol=1e-9) and np.allclose(nv["bn/batch_normalization"][0], [0.0, 0.99], atol=1e-9)
    assert np.array_equal(nv["bn/batch_normalization"][1:], var["bn/batch_normalization"][1:])
    assert np.allclose(nm["a"], [0.06, 0.0]) and np.allclose(nvv["a"], [0.00036, 0.0])
    small = {k: 0.1 * v for k, v in grads.items()}          # below the clip norm: not scaled
    assert np.array_equal(SG.train_step(var, small, zeros, zeros, 1, 0.01, 0.9, 0.999)[4]["a"], small["a"])


# ---------------------------------------------------------------- the schedule (tacotron.py:292-303)
def test_learning_rate_known_answers():
    import torch_tacotron_speaker_grad_ref as SG
    from twvk_amd.tacotron_train import learning_rate
    lr0 = 1e-3
    for random_init, w in ((True, 4000.0), (False, 40000.0)):
        want = {1: lr0 / w, 4000: lr0 * 4000.0 / w if w > 4000 else lr0, 4001: lr0 * 4001.0 / w if w > 4001 else lr0 * (4000.0 / 4001.0) ** 0.5,
                int(w): lr0}
        for step, v in want.items():
            assert learning_rate(lr0, step, 0, random_init) == pytest.approx(v, rel=1e-12), (random_init, step)
            assert SG.learning_rate(lr0, step, 0, random_init) == pytest.approx(v, rel=1e-12)
        # the peak: lr0 at step = w, below it on both sides
        assert learning_rate(lr0, w - 1, 0, random_init) < lr0 > learning_rate(lr0, w + 1, 0, random_init)
    assert learning_rate(lr0, 1, 1) == pytest.approx(lr0 * 0.95 ** (1.0 / 3000.0), rel=1e-12)
    assert learning_rate(lr0, 3000, 1) == pytest.approx(lr0 * 0.95, rel=1e-12)
    assert SG.learning_rate(lr0, 3000, 1, True) == pytest.approx(lr0 * 0.95, rel=1e-12)
    assert learning_rate(lr0, 3000, 1, False) == learning_rate(lr0, 3000, 1, True)
    with pytest.raises(ValueError):
        learning_rate(lr0, 1, 2)


# ---------------------------------------------------------------- the training vector
@pytest.mark.parametrize("speakers, kw", [(2, {}), (1, {}), (2, dict(speaker_embedding_size=1)), (2, dict(enc_bank_channel_size=30, post_bank_channel_size=30))])
def test_training_vector_layout(speakers, kw):
    import torch_attention_ref as AR
    from twvk_amd.tacotron import flatten, flatten_variables, speaker_grad_layout, training_layout
    m = _model(speakers, **kw)
    layout = training_layout(m.specs)
    n = int(m._L.twv_tacotron_train_floats(m._h))
    bn = sum(2 * shp[1] for name, shp in m.specs if name.endswith("batch_normalization"))
    assert bn > 0 and n == int(m._L.twv_tacotron_blob_floats(m._h)) + bn == sum(int(np.prod(s)) for _, _, s in layout)
    # every name once, in the canonical order, the ranges back to back
    assert [a for a, _, _ in layout] == [a for a, _ in m.specs] and len({a for a, _, _ in layout}) == len(layout)
    assert layout[0][1] == 0 and all(o0 + int(np.prod(s0)) == o1 for (_, o0, s0), (_, o1, _) in zip(layout, layout[1:]))
    w = AR.random_tensors(m.specs, seed=7)
    flat = flatten_variables(m.specs, w)
    back = {a: flat[o:o + int(np.prod(s))].reshape(s) for a, o, s in layout}
    assert flat.size == n and all(np.array_equal(back[a], w[a]) for a in w)
    assert np.array_equal(flatten(m.specs, back), flatten(m.specs, w))
    spk = [a for a, _, _ in speaker_grad_layout(m.specs)]
    assert len(spk) == (0 if speakers == 1 else (3 + m._hparams.dec_layer_num) * (1 if "speaker_embedding_size" in kw else 2) + (0 if "speaker_embedding_size" in kw else 1))


# ---------------------------------------------------------------- the C entries
def test_entry_points_exist():
    from twvk_amd import _lib
    header = open(os.path.join(ROOT, "include", "twv_amd.h")).read()
    declared = set(re.findall(r"\b(twv_[a-z0-9_]+)\s*\(", header))
    L = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert set(_lib.EXPORTS) <= declared
    import twvk_amd
    from twvk_amd.tacotron import Tacotron
    assert twvk_amd.TacotronTrainer.step and Tacotron.speaker_grad and Tacotron.variable_gradients


SPEAKER_ARGS = ("h", "blob", "speaker_ids", "d_before_highway", "d_encoder_rnn_init", "d_init", "scratch", "grad_blob")


def _speaker_grad(m, null=None, batch=3):
    from twvk_amd import _lib
    buf = (C.c_float * 16)()                     # a host address: every refusal comes before anything is read
    p = C.cast(buf, C.c_void_p)
    a = {n: (None if n == null else (m._h if n == "h" else p)) for n in SPEAKER_ARGS}
    _lib.check(m._L.twv_tacotron_speaker_grad(a["h"], a["blob"], a["speaker_ids"], batch, a["d_before_highway"], a["d_encoder_rnn_init"], a["d_init"],
                                              a["scratch"], a["grad_blob"], None))


@pytest.mark.parametrize("null", SPEAKER_ARGS)
def test_speaker_grad_refuses_null_arguments(null):
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 1: null argument"):
        _speaker_grad(_model(), null)


def test_speaker_grad_refuses_models_without_a_speaker_side():
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 1: .*single-speaker model has no speaker tensors"):
        _speaker_grad(_model(1))
    with pytest.raises(TwvError, match="twv_amd error 2: model_type 'simple': .*built for 'deepvoice' models"):
        _speaker_grad(_model(4, model_type="simple"))
    with pytest.raises(TwvError, match="twv_amd error 1: batch >= 1"):
        _speaker_grad(_model(), batch=0)
    m = _model()
    hp = m._hparams
    total = hp.enc_prenet_sizes[1] + 2 * hp.enc_rnn_size + hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size
    scratch = lambda mm, n: int(mm._L.twv_tacotron_speaker_grad_scratch_bytes(mm._h, n))
    assert scratch(m, 3) >= 4 * 3 * (total + hp.speaker_embedding_size) and scratch(m, 9) > scratch(m, 3)
    assert 0 < scratch(_model(speaker_embedding_size=1), 3) <= 64 and scratch(m, 0) == 0


def test_refold_and_grad_convert_refuse_null_arguments():
    from twvk_amd import _lib
    m = _model()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    for args in ((None, p, p), (m._h, None, p), (m._h, p, None)):
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(m._L.twv_tacotron_refold(args[0], args[1], args[2], None))
    for args in ((None, p, p, p), (m._h, None, p, p), (m._h, p, None, p), (m._h, p, p, None)):
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(m._L.twv_tacotron_grad_convert(args[0], args[1], args[2], args[3], None))
    assert m._L.twv_tacotron_train_floats(None) == 0


# ---------------------------------------------------------------- the conditions of the whole-model cases
@pytest.mark.parametrize("name", sorted(WHOLE))
def test_margin_condition_of_the_whole_model_cases(name):
    """tests/test_tacotron_cbhg_grad_cpu.py test_margin_condition_of_the_chain_cases on the cases of this table, over every tensor
    variable_vjp differentiates: the speaker tensors too"""
    import torch_tacotron_cbhg_grad_ref as CG
    import torch_tacotron_speaker_grad_ref as SG
    h = whole_case(name)
    _, g64, rec = whole_checker(name, "float64")
    _, g32, rec32 = whole_checker(name, "float32")
    assert CG.same_branches(rec, rec32) and rec["relu_margin"] > MARGIN and rec["pool_gap"] > MARGIN, (rec["relu_margin"], rec["pool_gap"])
    assert rec["loss_margin"] > 1e-5 and rec["cumprod_margin"] > 1e-3 and rec["min_one_minus_p"] >= np.finfo(np.float32).tiny, rec["loss_margin"]
    worst = max((float(np.abs(g32[k] - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-30), k) for k in g64)
    print("%s: worst e_t32 %.3e (%s)" % ((name,) + worst))
    assert worst[0] < CHAIN_E_T32, worst
    assert h.speakers > 1
    assert set(g64) == set(n for n, _ in h.specs) | {"d_init", "d_before_highway", "d_encoder_rnn_init"}


def test_twenty_checker_steps_lower_the_checker_loss():
    """the rate of the device's twenty-step test: twenty evaluation-graph steps of the float64 checker (variable_vjp + train_step) on
    C-length-one's fixed batch end below the first loss"""
    import torch
    import torch_tacotron_speaker_grad_ref as SG
    h = whole_case("C-length-one")
    hp = h.hp
    var = {k: np.asarray(v, np.float64) for k, v in h.w.items()}
    m = {k: np.zeros_like(v) for k, v in var.items()}
    v = {k: np.zeros_like(x) for k, x in var.items()}
    losses = []
    for t in range(1, TWENTY_STEPS + 2):
        loss, g, _ = SG.variable_vjp(var, h.specs, h.dims, h.tok, h.ln, h.spk, h.at, h.tgt, h.lin_tgt, h.coeff, hp.prioritize_loss, hp.sample_rate,
                                     hp.num_freq, dtype=torch.float64)
        losses.append(loss)
        if t <= TWENTY_STEPS:
            var, m, v, _, _ = SG.train_step(var, g, m, v, t, SG.learning_rate(TWENTY_LR0, t, TWENTY_MODE, False), hp.adam_beta1, hp.adam_beta2)
    print("checker losses:", " ".join("%.5f" % x for x in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
