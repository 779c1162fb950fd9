"""-m gpu: the whole model at the softmax attention types and loc_sen, one case per new kind (tests/tacotron_attention_grad_cases.py WHOLE):
Tacotron.variable_gradients with attention_gradients="any" against the whole-model checker under the gradient bar, one
TacotronTrainer(..., attention_gradients="any") step in both graphs held to the bars of tests/test_tacotron_train_gpu.py and
tests/test_tacotron_trainmode_gpu.py (imported from there, not restated), save -> restore -> the next step, Synthesizer.load -> infer, and
train_tacotron.main on a loc_sen model."""
import functools

import numpy as np
import pytest

from helpers import assert_bar, first_mismatch, same_outputs
from tacotron_attention_grad_cases import WHOLE, WholeCase
from tacotron_grad_cases import SMALL, hparams
from test_tacotron_train_gpu import STEP_ATOL, STEP_LR0

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    import torch
    assert torch.cuda.is_available()
    return WholeCase(name)


def _model(h, **kw):
    from twvk_amd.tacotron import Tacotron
    hp = hparams(max_iters=8, **dict(SMALL, attention_type=h.at, **kw))
    m = Tacotron(hp, num_speakers=h.speakers)
    m.load_weights(h.w)
    return m


def _trainer(h, training=False, seed=7):
    from twvk_amd.tacotron_train import TacotronTrainer
    m = _model(h, tacotron_initial_learning_rate=STEP_LR0, decay_learning_rate_mode=1)
    return (TacotronTrainer(m, training=training, seed=seed, attention_gradients="any"), (h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, h.coeff))


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_variable_gradients_against_the_whole_model_checker(name):
    from twvk_amd._lib import TwvError
    h = _case(name)
    ok, fig = h.whole_conditions()
    assert ok, fig
    m = _model(h)
    m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=True)
    loss = m.add_loss(h.lin_tgt, h.coeff)["loss"]
    with pytest.raises(TwvError, match="twv_amd error 2: .*attention_type"):      # the default door stays shut
        m.variable_gradients(h.lin_tgt, h.coeff)
    m.attention_gradients = "any"
    got = {k: v.cpu().numpy() for k, v in m.variable_gradients(h.lin_tgt, h.coeff).items()}
    assert m.decoder_grad_route().startswith("kernel=tg_bptt attention=%s " % h.at)
    l64, g64, _ = h.checker("float64")
    _, g32, _ = h.checker("float32")
    assert set(got) == set(g64) == set(n for n, _ in h.specs) | {"d_init", "d_before_highway", "d_encoder_rnn_init"}, set(got) ^ set(g64)
    assert abs(loss - l64) <= 1e-4 * abs(l64)
    assert_bar(name + " variables", got, g64, g32)


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_one_step_in_both_graphs_save_restore_and_synthesizer(name, tmp_path):
    """the evaluation-graph step as tests/test_tacotron_train_gpu.py::test_one_step_against_the_checker_update holds it (variables within
    STEP_ATOL * lr / 1e-3 of float64 clip + Adam fed the device's gradients), the training-graph step to the same bar with the moving
    statistics within 1e-6 of the float64 formula on the float64 checker's statistics (tests/test_tacotron_trainmode_gpu.py)"""
    import torch
    import torch_tacotron_speaker_grad_ref as SG
    import torch_tacotron_trainmode_ref as TM
    from twvk_amd.synthesizer import Synthesizer
    from twvk_amd.tacotron import Tacotron, flatten
    from twvk_amd.tacotron_train import TacotronTrainer
    h = _case(name)
    hp = h.hp
    lr = SG.learning_rate(STEP_LR0, 1, 1, True)
    atol = STEP_ATOL * (lr / 1e-3)
    for training in (False, True):
        t, batch = _trainer(h, training=training)
        before = t.variables()
        losses = t.loss_and_gradients(*batch)
        raw = t.gradients()
        assert all(np.isfinite(v).all() for v in raw.values())
        used = t.apply_gradients()
        assert t.global_step == 1 and used == pytest.approx(lr, rel=1e-12)
        after = t.variables()
        zeros = {k: np.zeros(np.shape(v)) for k, v in before.items()}
        want, _, _, norm, _ = SG.train_step(before, raw, zeros, zeros, 1, lr, hp.adam_beta1, hp.adam_beta2)
        bn = lambda k: k.endswith("batch_normalization")
        worst = max((float(np.abs(after[k][:2].astype(np.float64) - want[k][:2]).max()) if bn(k) else float(np.abs(after[k].astype(np.float64) - want[k]).max()), k)
                    for k in want)
        print("%s training=%s: gradient norm %.4f, worst |variable - checker| %.3e (%s), bar %.3e" % (name, training, norm, worst[0], worst[1], atol))
        assert worst[0] <= atol, worst
        if training:
            masks = [m_.cpu().numpy() for m_ in t.last_masks]
            s64 = TM.variable_vjp(h.w, h.specs, h.dims, h.tok, h.ln, h.spk, h.at, h.tgt, h.lin_tgt, h.coeff, hp.prioritize_loss, hp.sample_rate, hp.num_freq,
                                  masks=masks, dtype=torch.float64)[3]
            worst_m = 0.0
            for k, s in s64.items():
                mv = TM.moving_average(before[k][2:], s)
                worst_m = max(worst_m, float(np.abs(after[k][2:] - mv).max()) / float(np.abs(mv).max()))
            print("%s: moving statistics against the float64 formula: worst %.3e of a tensor's maximum" % (name, worst_m))
            assert worst_m <= 1e-6, worst_m
        else:
            for k in after:
                if bn(k):
                    assert first_mismatch(after[k][2:], before[k][2:]) is None, k
        assert first_mismatch(t.model._blob.cpu().numpy(), flatten(t.model.specs, after)) is None
        # save -> restore -> the next step: the uninterrupted run's bits
        d = tmp_path / ("training" if training else "evaluation")
        d.mkdir()
        assert t.save(str(d)).endswith("model.ckpt-1")
        inferred = [a.cpu().numpy() for a in t.model.infer(h.tok, h.ln, h.spk)]
        nxt = t.step(*batch)
        t2 = TacotronTrainer(Tacotron(t.model._hparams, num_speakers=h.speakers), training=training, seed=7, attention_gradients="any")
        assert t2.restore(str(d)) == 1
        same_outputs(after, t2.variables(), "restored variables")
        assert t2.step(*batch) == nxt and t2.global_step == 2
        same_outputs(t.variables(), t2.variables(), "the step after the restore")
        # the bundle is a checkpoint Synthesizer.load reads
        s = Synthesizer()
        s.load(str(d), num_speakers=h.speakers, hparams=t.model._hparams)
        for a, b in zip(inferred, s.model.infer(h.tok, h.ln, h.spk)):
            assert first_mismatch(a, b.cpu().numpy()) is None
    assert losses["loss"] > 0.0


def test_twenty_training_mode_steps_of_loc_sen():
    """twenty steps on whole-loc_sen's fixed batch against the float64 checker's own twenty steps, as
    tests/test_tacotron_trainmode_gpu.py::test_twenty_training_mode_steps_and_a_restore: the loss falls in both, and the device ends within
    TWENTY_STEPS * STEP_ATOL * (lr0 / 1e-3) * sum |d loss / d variable| of the checker (that test's margin; its constants are imported)"""
    import torch
    import torch_tacotron_speaker_grad_ref as SG
    import torch_tacotron_trainmode_ref as TM
    from tacotron_trainmode_cases import STEP_SEED, TWENTY_LR0, TWENTY_MODE, TWENTY_STEPS
    from twvk_amd.tacotron import Tacotron, dropout_mask_numpy
    from twvk_amd.tacotron_train import TacotronTrainer
    h = _case("whole-loc_sen")
    hp = h.hp
    m = _model(h, tacotron_initial_learning_rate=TWENTY_LR0, decay_learning_rate_mode=TWENTY_MODE)
    t = TacotronTrainer(m, randomly_initialized=False, training=True, seed=STEP_SEED, attention_gradients="any")
    batch = (h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, h.coeff)
    losses = [t.step(*batch)["loss"] for _ in range(TWENTY_STEPS)]
    steps = h.TO // hp.reduction_factor
    shapes = [(h.N, h.T, hp.enc_prenet_sizes[0]), (h.N, h.T, hp.enc_prenet_sizes[1]), (h.N, steps, hp.dec_prenet_sizes[0]), (h.N, steps, hp.dec_prenet_sizes[1])]
    masks = lambda k: [dropout_mask_numpy(int(np.prod(sh)), STEP_SEED, k, site, 0.5).reshape(sh) for site, sh in enumerate(shapes)]
    l64, _, g1 = TM.train_steps(h.w, h.specs, h.dims, batch, masks, lambda s_: SG.learning_rate(TWENTY_LR0, s_, TWENTY_MODE, False), hp.adam_beta1,
                                hp.adam_beta2, TWENTY_STEPS, hp.prioritize_loss, hp.sample_rate, hp.num_freq, h.at, dtype=torch.float64)
    margin = TWENTY_STEPS * STEP_ATOL * (TWENTY_LR0 / 1e-3) * g1
    print("device   :", " ".join("%.6f" % x for x in losses))
    print("float64  :", " ".join("%.6f" % x for x in l64))
    print("step 20: device %.7f, float64 checker %.7f, difference %.3e; sum |gradient| %.3f, margin %.3e" % (losses[-1], l64[-1], abs(losses[-1] - l64[-1]), g1, margin))
    assert np.isfinite(losses).all() and losses[-1] < losses[0] and l64[-1] < l64[0], (losses, l64)
    assert abs(losses[-1] - l64[-1]) <= margin, (losses[-1], l64[-1], margin)


def test_train_tacotron_trains_a_loc_sen_model(tmp_path):
    import os
    from tacotron_feed_cases import write_directories
    from test_train_tacotron_gpu import _hp, _run
    hp = lambda: _hp(attention_type="loc_sen")
    dirs = write_directories(tmp_path / "data", hp(), speakers=2, per_speaker=12, seed=3, frames=(6, 34), tokens=(3, 12))
    common = ["--data_paths", ",".join(dirs), "--batch_size", "3", "--random_seed", "7", "--summary_interval", "2", "--test_interval", "3",
              "--checkpoint_interval", "3"]
    out, lines = _run(["--log_dir", str(tmp_path / "logs")] + common + ["--num_steps", "3"], hp())
    d = out["model_dir"]
    assert out["step"] == 3 and len(out["losses"]) == 3 and np.isfinite(out["losses"]).all()
    assert out["trainer"].model.decoder_grad_route().startswith("kernel=tg_bptt attention=loc_sen ")
    for suffix in (".index", ".data-00000-of-00001"):
        assert os.path.exists(os.path.join(d, "model.ckpt-3" + suffix))
    # the same seed: the same bytes
    out2, _ = _run(["--log_dir", str(tmp_path / "logs2")] + common + ["--num_steps", "3"], hp())
    assert out2["losses"] == out["losses"]
    for suffix in (".index", ".data-00000-of-00001"):
        a, b = (open(os.path.join(x["model_dir"], "model.ckpt-3" + suffix), "rb").read() for x in (out, out2))
        assert a == b, suffix
    # --load_path continues at step 4
    out3, lines3 = _run(["--load_path", d] + common + ["--num_steps", "5"], hp())
    assert out3["model_dir"] == d and out3["step"] == 5 and [l.split()[1] for l in lines3 if l.startswith("Step ")] == ["4", "5"]
