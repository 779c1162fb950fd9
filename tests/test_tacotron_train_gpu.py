"""-m gpu: the Tacotron training step.  twv_tacotron_speaker_grad against the float64 checker
tests/torch_tacotron_speaker_grad_ref.py under the project's gradient bar (tests/train_cases.py RATIO / FLOOR) and its exact properties;
twv_tacotron_refold against tacotron.flatten bit for bit and twv_tacotron_grad_convert against tacotron.bn_grad_from_inference_pair;
Tacotron.variable_gradients against the whole-model checker; one TacotronTrainer.step against the checker's update rule fed the device's
gradients; twenty steps, a save / restore and a Synthesizer.load of the result.

The cases are tests/tacotron_train_cases.py, whose conditions tests/test_tacotron_train_cpu.py proves on the host."""
import functools

import numpy as np
import pytest

from helpers import assert_bar, first_mismatch, same_outputs
from tacotron_cbhg_grad_cases import CASES
from tacotron_train_cases import SPEAKER_CASES, TWENTY_LR0, TWENTY_MODE, TWENTY_STEPS, WHOLE, hparams, SMALL, speaker_case, whole_case, whole_checker

pytestmark = pytest.mark.gpu

STEP_LR0 = 1e-3          # tacotron_initial_learning_rate of the one-step test, with mode 1: lr = 1e-3 * 0.95^(1/3000) = 0.99998e-3 at step 1
STEP_ATOL = 2e-6         # the WaveNet step's bar at lr 1e-3 (tests/test_train_gpu.py); scaled by lr / 1e-3 below


def _zero_bits(a):
    return not np.ascontiguousarray(a, np.float32).view(np.uint32).any()


def _model(hp, speakers, w):
    import torch
    from twvk_amd.tacotron import Tacotron
    assert torch.cuda.is_available()
    m = Tacotron(hp, num_speakers=speakers)
    m.load_weights(w)
    return m


# ---------------------------------------------------------------- speaker_grad in isolation
class _Speaker(object):
    def __init__(self, name):
        self.c = speaker_case(name)
        self.m = _model(self.c.hp, self.c.speakers, self.c.w)

    def run(self, cot=None, poison=False):
        """the C entry on a gradient buffer and scratch filled with NaN (poison) or zeros: ({name: gradient}, the words outside the speaker ranges)"""
        import torch
        from twvk_amd import _lib
        from twvk_amd.tacotron import _ptr, _stream, speaker_grad_layout
        c, m, dev = self.c, self.m, self.m.device
        fill = float("nan") if poison else 0.0
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d = [up(a) for a in (c.cot if cot is None else cot)]
        ids = up(c.ids)
        with torch.cuda.device(dev):
            grad = torch.full_like(m._blob, fill)
            scratch = torch.full((m._L.twv_tacotron_speaker_grad_scratch_bytes(m._h, c.N) // 4,), fill, dtype=torch.float32, device=dev)
            _lib.check(m._L.twv_tacotron_speaker_grad(m._h, _ptr(m._blob), _ptr(ids), c.N, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(scratch), _ptr(grad),
                                                      _stream()))
            torch.cuda.synchronize()
        g = grad.cpu().numpy()
        out, inside = {}, np.zeros(g.size, bool)
        for name, off, shp in speaker_grad_layout(m.specs):
            out[name] = g[off:off + int(np.prod(shp))].reshape(shp).copy()
            inside[off:off + out[name].size] = True
        return out, g[~inside]

    @functools.lru_cache(maxsize=None)
    def first(self):
        return self.run()


@functools.lru_cache(maxsize=None)
def _speaker(name):
    return _Speaker(name)


@pytest.mark.parametrize("name", sorted(SPEAKER_CASES))
def test_speaker_gradients_meet_the_bar(name):
    import torch_tacotron_speaker_grad_ref as SG
    s = _speaker(name)
    c = s.c
    got, outside = s.first()
    g64, g32 = c.checker("float64"), c.checker("float32")
    assert set(got) == set(g64) == set(SG.speaker_names(c.w, c.dims)), set(got) ^ set(g64)
    assert_bar(name + " speaker", got, g64, g32)
    assert not outside.any()                                  # (the zero fill of this run: the call wrote nothing there)
    # a speaker no utterance names: a row of zero bits in every table; a named one has a gradient
    unnamed = sorted(set(range(c.speakers)) - set(int(i) for i in c.ids))
    assert unnamed or "unnamed" not in name
    for k in (["speaker_embedding"] if "speaker_embedding" in got else sorted(got)):
        for sp in range(c.speakers):
            assert _zero_bits(got[k][sp]) == (sp in unnamed), (name, k, sp)


@pytest.mark.parametrize("name", ["a-three", "b-nine-unnamed-speaker", "d-tables"])
def test_speaker_gradients_exact_properties(name):
    s = _speaker(name)
    c = s.c
    one, _ = s.first()
    two, _ = s.run(cot=[2.0 * a for a in c.cot])
    zero, _ = s.run(cot=[np.zeros_like(a) for a in c.cot])
    for k in one:                                             # linear in the cotangent, bit for bit
        assert first_mismatch(2.0 * one[k], two[k]) is None, (name, k)
        assert not zero[k].any(), (name, k)
    same_outputs(one, s.run()[0], name + " second run")
    poisoned, outside = s.run(poison=True)
    assert all(np.isfinite(v).all() for v in poisoned.values()), name
    same_outputs(one, poisoned, name + " NaN-filled scratch and gradient buffer")
    assert outside.size and np.isnan(outside).all(), name    # nothing outside the speaker tensors' ranges was written


# ---------------------------------------------------------------- variables <-> blob
@functools.lru_cache(maxsize=None)
def _fold_case(odd):
    """a random model with the moving variances spread over four decades, its training vector on the device"""
    import torch
    import torch_attention_ref as AR
    from twvk_amd.tacotron import flatten_variables
    kw = dict(enc_bank_channel_size=30, post_bank_channel_size=30, speaker_embedding_size=1) if odd else {}
    hp = hparams(max_iters=8, **dict(SMALL, **kw))
    from twvk_amd.tacotron import tacotron_specs
    specs = tacotron_specs(hp, 2)
    w = AR.random_tensors(specs, seed=41 + odd)
    rng = np.random.RandomState(43 + odd)
    for k in w:
        if k.endswith("batch_normalization"):
            c = w[k].shape[1]
            w[k] = np.stack([rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c), rng.randn(c), rng.randn(c), 10.0 ** rng.uniform(-3.0, 1.0, c)]).astype(np.float32)
    m = _model(hp, 2, w)
    var = torch.from_numpy(flatten_variables(specs, w)).to(m.device)
    return m, w, var


@pytest.mark.parametrize("odd", [0, 1])
def test_refold_is_flatten_bit_for_bit(odd):
    import torch
    from twvk_amd import _lib
    from twvk_amd.tacotron import _ptr, _stream, flatten
    m, w, var = _fold_case(odd)
    assert var.numel() == m._L.twv_tacotron_train_floats(m._h)
    with torch.cuda.device(m.device):
        blob = torch.full_like(m._blob, float("nan"))
        _lib.check(m._L.twv_tacotron_refold(m._h, _ptr(var), _ptr(blob), _stream()))
        torch.cuda.synchronize()
    want = flatten(m.specs, w)
    got = blob.cpu().numpy()
    assert first_mismatch(got, want) is None, first_mismatch(got, want)
    assert first_mismatch(got, m._blob.cpu().numpy()) is None


@pytest.mark.parametrize("odd", [0, 1])
def test_grad_convert_against_bn_grad_from_inference_pair(odd):
    import torch
    from twvk_amd import _lib
    from twvk_amd.tacotron import BN_EPS, _grad_layout, _ptr, _stream, bn_grad_from_inference_pair, training_layout
    m, w, var = _fold_case(odd)
    rng = np.random.RandomState(47)
    g = rng.randn(m._blob.numel()).astype(np.float32)
    with torch.cuda.device(m.device):
        gb = torch.from_numpy(g).to(m.device)
        out = torch.full_like(var, float("nan"))
        _lib.check(m._L.twv_tacotron_grad_convert(m._h, _ptr(var), _ptr(gb), _ptr(out), _stream()))
        torch.cuda.synchronize()
    got = out.cpu().numpy()
    blob_at = {n: (off, shp) for n, off, shp in _grad_layout(m.specs, lambda i, n: True)}
    seen = 0
    for name, off, shp in training_layout(m.specs):
        mine = got[off:off + int(np.prod(shp))].reshape(shp)
        boff, bshp = blob_at[name]
        src = g[boff:boff + int(np.prod(bshp))].reshape(bshp)
        if name.endswith("batch_normalization"):
            seen += 1
            want = bn_grad_from_inference_pair(src, w[name])
            raw = np.asarray(w[name], np.float64)
            rs = 1.0 / np.sqrt(raw[3] + np.float64(BN_EPS))
            # one float32 rounding of a float64 expression evaluated in either association
            bound = 2.0 ** -23 * rs * (np.abs(src[0].astype(np.float64)) + np.abs(raw[2] * src[1]))
            assert (np.abs(mine[0].astype(np.float64) - want[0]) <= bound).all(), name
            assert first_mismatch(mine[1], src[1]) is None, name
            assert _zero_bits(mine[2:]), name
        else:
            assert first_mismatch(mine, src) is None, name
    assert seen == sum(1 for n, _ in m.specs if n.endswith("batch_normalization")) > 0


# ---------------------------------------------------------------- the whole model
class _Whole(object):
    def __init__(self, name):
        self.h = whole_case(name)
        self.m = _model(self.h.hp, self.h.speakers, self.h.w)

    @functools.lru_cache(maxsize=None)
    def gradients(self):
        h, m = self.h, self.m
        m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=True)
        loss = m.add_loss(h.lin_tgt, h.coeff)["loss"]
        return loss, {k: v.cpu().numpy() for k, v in m.variable_gradients(h.lin_tgt, h.coeff).items()}


@functools.lru_cache(maxsize=None)
def _whole(name):
    return _Whole(name)


@pytest.mark.parametrize("name", sorted(WHOLE))
def test_variable_gradients_against_the_whole_model_checker(name):
    w = _whole(name)
    h, m = w.h, w.m
    loss, got = w.gradients()
    l64, g64, _ = whole_checker(name, "float64")
    _, g32, _ = whole_checker(name, "float32")
    assert set(got) == set(g64) == set(n for n, _ in h.specs) | {"d_init", "d_before_highway", "d_encoder_rnn_init"}, set(got) ^ set(g64)
    assert abs(loss - l64) <= 1e-4 * abs(l64)
    assert_bar(name + " variables", got, g64, g32)
    # loss_gradients keeps its key set, and speaker_grad is the rest
    base = m.loss_gradients(h.lin_tgt, h.coeff)
    spk = m.speaker_grad(base["d_before_highway"], base["d_encoder_rnn_init"], base["d_init"])
    assert set(base) | set(spk) == set(got) and not set(base) & set(spk)
    for k, v in list(base.items()) + list(spk.items()):
        assert first_mismatch(v.cpu().numpy(), got[k]) is None, k


def _trainer(h, lr0, mode, randomly_initialized=True, coeff_scale=1.0):
    from twvk_amd.tacotron_train import TacotronTrainer
    hp = hparams(max_iters=8, **dict(SMALL, tacotron_initial_learning_rate=lr0, decay_learning_rate_mode=mode, **CASES[h.name][5]))
    m = _model(hp, h.speakers, h.w)
    return TacotronTrainer(m, randomly_initialized=randomly_initialized), (h.tok, h.ln, h.spk, h.tgt, h.lin_tgt, coeff_scale * h.coeff)


@pytest.mark.parametrize("name, coeff_scale", [("C-length-one", 1.0), ("C-length-one", 8.0), ("F-speaker-tables", 8.0)])
def test_one_step_against_the_checker_update(name, coeff_scale):
    """lr = 1e-3 * 0.95^(1/3000) (mode 1, step 1): the updated variables within 2e-6 * (lr / 1e-3) of clip + Adam in float64 fed the device's
    gradients.  coeff_scale 8 lifts the gradient's norm (0.27 at the case's own loss_coeff) above the clip norm."""
    import torch_tacotron_speaker_grad_ref as SG
    from twvk_amd.tacotron import flatten
    h = whole_case(name)
    t, batch = _trainer(h, STEP_LR0, 1, coeff_scale=coeff_scale)
    m = t.model
    lr = SG.learning_rate(STEP_LR0, 1, 1, True)
    before = t.variables()
    assert all(first_mismatch(before[k], h.w[k]) is None for k in h.w) and t.global_step == 0
    losses = t.loss_and_gradients(*batch)
    raw = t.gradients()                                       # (before the clip)
    assert all(np.isfinite(v).all() for v in raw.values())
    m.forward_targets(*batch[:4], teacher_forced=True)
    assert losses == m.add_loss(batch[4], batch[5])
    used = t.apply_gradients()
    assert t.global_step == 1 and used == pytest.approx(lr, rel=1e-12) == pytest.approx(t.learning_rate(1), rel=1e-12)
    after, clipped = t.variables(), t.gradients()
    zeros = {k: np.zeros(np.shape(v)) for k, v in before.items()}
    want, _, _, norm, want_clipped = SG.train_step(before, raw, zeros, zeros, 1, lr, h.hp.adam_beta1, h.hp.adam_beta2)
    print("%s x%g: raw gradient norm %.6f lr %.9e" % (name, coeff_scale, norm, lr))
    assert (norm > 1.0) == (coeff_scale > 1.0), norm
    got_norm = float(np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in clipped.values())))
    if norm > 1.0:
        assert got_norm == pytest.approx(1.0, rel=1e-5), got_norm
    else:
        assert all(first_mismatch(clipped[k], raw[k]) is None for k in raw)
    atol = STEP_ATOL * (lr / 1e-3)
    worst = max((float(np.abs(after[k].astype(np.float64) - want[k]).max()), k) for k in want)
    print("%s x%g: worst |variable - checker| %.3e (%s), bar %.3e" % (name, coeff_scale, worst[0], worst[1], atol))
    assert worst[0] <= atol, worst
    for k in after:
        if k.endswith("batch_normalization"):                 # the moving statistics: the same bits, whatever gamma and beta did
            assert first_mismatch(after[k][2:], before[k][2:]) is None and _zero_bits(clipped[k][2:]), k
        # Adam's first step moves an element by lr * g / (|g| + 1e-8): about lr where the gradient is not tiny, not at all where it is zero
        assert not (after[k] != before[k])[raw[k] == 0.0].any() and (after[k] != before[k])[np.abs(clipped[k]) > 1e-6].all(), k
    assert all(raw[k].any() for k in raw)
    # the model's blob is host flatten of the variables, and its passes see the new weights
    assert first_mismatch(m._blob.cpu().numpy(), flatten(m.specs, after)) is None
    mel = m.forward_targets(*batch[:4], teacher_forced=True)[0].cpu().numpy()
    fresh = _model(m._hparams, h.speakers, after)
    assert first_mismatch(fresh.forward_targets(*batch[:4], teacher_forced=True)[0].cpu().numpy(), mel) is None
    assert m.add_loss(batch[4], batch[5])["loss"] != losses["loss"]
    # a second trainer from the same weights, through step(): the same bits
    t2, _ = _trainer(h, STEP_LR0, 1, coeff_scale=coeff_scale)
    assert t2.step(*batch) == losses and t2.global_step == 1 and t2.last_learning_rate == used
    same_outputs(after, t2.variables(), name + " second trainer")
    assert first_mismatch(t2.model._blob.cpu().numpy(), m._blob.cpu().numpy()) is None


def test_schedule_of_mode_zero_follows_global_step():
    import torch_tacotron_speaker_grad_ref as SG
    h = whole_case("C-length-one")
    for random_init in (True, False):
        t, batch = _trainer(h, 2e-3, 0, randomly_initialized=random_init)
        for step in (1, 2):
            t.step(*batch)
            assert t.global_step == step and t.last_learning_rate == pytest.approx(SG.learning_rate(2e-3, step, 0, random_init), rel=1e-12)


def test_twenty_steps_save_restore_and_synthesizer(tmp_path):
    """twenty steps on C-length-one's fixed batch at tacotron_initial_learning_rate 1e-3, mode 1, randomly_initialized=False (the rate at
    which the float64 checker's own loss falls: tests/test_tacotron_train_cpu.py)"""
    from twvk_amd.synthesizer import Synthesizer
    from twvk_amd.tacotron import Tacotron
    from twvk_amd.tacotron_train import TacotronTrainer
    h = whole_case("C-length-one")
    t, batch = _trainer(h, TWENTY_LR0, TWENTY_MODE, randomly_initialized=False)
    losses = [t.step(*batch)["loss"] for _ in range(TWENTY_STEPS)]
    prefix = t.save(str(tmp_path))
    assert prefix.endswith("model.ckpt-%d" % TWENTY_STEPS) and t.global_step == TWENTY_STEPS
    trained = t.variables()
    inferred = [a.cpu().numpy() for a in t.model.infer(h.tok, h.ln, h.spk)]
    nxt = t.step(*batch)
    losses.append(nxt["loss"])
    print("losses:", " ".join("%.5f" % x for x in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert all(np.isfinite(v).all() for v in t.variables().values())
    # a fresh model and trainer from the bundle: the next step is the uninterrupted run's, bit for bit
    hp = t.model._hparams
    t2 = TacotronTrainer(Tacotron(hp, num_speakers=h.speakers), randomly_initialized=False)
    assert t2.restore(str(tmp_path)) == TWENTY_STEPS == t2.global_step
    same_outputs(trained, t2.variables(), "restored variables")
    assert t2.step(*batch) == nxt and t2.global_step == TWENTY_STEPS + 1
    same_outputs(t.variables(), t2.variables(), "the step after the restore")
    # the bundle is a checkpoint Synthesizer.load reads
    s = Synthesizer()
    s.load(str(tmp_path), num_speakers=h.speakers, hparams=hp)
    for a, b in zip(inferred, s.model.infer(h.tok, h.ln, h.spk)):
        assert first_mismatch(a, b.cpu().numpy()) is None


def test_a_single_speaker_model_has_no_speaker_side():
    """variable_gradients is loss_gradients there, and speaker_grad is the library's refusal"""
    from tacotron_cbhg_grad_cases import host_case
    from twvk_amd._lib import TwvError
    h = host_case("E-single-speaker")
    m = _model(h.hp, h.speakers, h.w)
    m.forward_targets(h.tok, h.ln, h.spk, h.tgt, teacher_forced=True)
    base, got = m.loss_gradients(h.lin_tgt, h.coeff), m.variable_gradients(h.lin_tgt, h.coeff)
    assert set(got) == set(base) == set(n for n, _ in h.specs) | {"d_init"}
    for k in base:
        assert first_mismatch(base[k].cpu().numpy(), got[k].cpu().numpy()) is None, k
    hp = h.hp
    zeros = [np.zeros((h.N, n), np.float32) for n in (hp.enc_prenet_sizes[1], 2 * hp.enc_rnn_size, hp.attention_state_size + hp.dec_layer_num * hp.dec_rnn_size)]
    with pytest.raises(TwvError, match="twv_amd error 1: .*single-speaker model has no speaker tensors"):
        m.speaker_grad(*zeros)
