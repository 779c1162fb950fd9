"""-m "not gpu": the host side of the Tacotron passes with mel targets -- exported symbols, every refusal of twv_tacotron_forward_targets /
twv_tacotron_loss (returned before a device is looked at), eval_tacotron's batching, skip rule and argument parser."""
import ctypes as C

import numpy as np
import pytest


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


@pytest.fixture(scope="module")
def model():
    from twvk_amd.tacotron import Tacotron
    return Tacotron(_hp(max_iters=8, enc_bank_size=4, post_bank_size=3, num_freq=129), num_speakers=2)       # r = 5


def test_symbols_are_exported_and_declared():
    import os
    from twvk_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    L = _lib.lib()
    for name in ("twv_tacotron_forward_targets", "twv_tacotron_loss"):
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in header, name


def _forward(model, t_out, teacher_forced, targets=True, null=None):
    """the C entry with dummy (never dereferenced) non-null pointers; `null` names the argument passed as NULL"""
    from twvk_amd import _lib
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = {n: p for n in ("packed", "tokens", "lengths", "speaker_ids", "workspace", "mel", "linear", "alignments", "status")}
    h = model._h
    if null == "h":
        h = None
    elif null:
        a[null] = None
    rc = model._L.twv_tacotron_forward_targets(h, a["packed"], a["tokens"], a["lengths"], a["speaker_ids"], 3, 19, p if targets else None,
                                               t_out, teacher_forced, a["workspace"], a["mel"], a["linear"], a["alignments"], a["status"], None)
    _lib.check(rc)


@pytest.mark.parametrize("t_out, teacher_forced, targets, null, message", [
    (23, 0, True, None, "multiple of reduction_factor"),            # t_out % r
    (0, 0, True, None, "1 <= steps <= max_iters"),                  # steps = 0
    (45, 1, True, None, "1 <= steps <= max_iters"),                 # steps = 9 > max_iters = 8
    (25, 1, False, None, "teacher_forced needs mel_targets"),
    (25, 0, True, "h", "null handle"),
    (25, 0, True, "packed", "null argument"),
    (25, 0, True, "tokens", "null argument"),
    (25, 0, True, "lengths", "null argument"),
    (25, 0, True, "workspace", "null argument"),
    (25, 0, True, "mel", "null argument"),
    (25, 0, True, "status", "null argument"),
])
def test_forward_targets_refusals(model, t_out, teacher_forced, targets, null, message):
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 1: .*" + message):          # TWV_E_INVALID
        _forward(model, t_out, teacher_forced, targets, null)


@pytest.mark.parametrize("null", ["mel", "linear", "mel_targets", "linear_targets", "out"])
def test_loss_refuses_null_pointers(model, null):
    from twvk_amd import _lib
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = {n: (None if n == null else p) for n in ("mel", "linear", "mel_targets", "linear_targets", "out")}
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
        _lib.check(model._L.twv_tacotron_loss(a["mel"], a["linear"], a["mel_targets"], a["linear_targets"], p, 3, 25, 80, 129, 0, 24000.0,
                                              a["out"], None))


def test_loss_refuses_a_null_loss_coeff(model):
    from twvk_amd import _lib
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: loss_coeff is required"):
        _lib.check(model._L.twv_tacotron_loss(p, p, p, p, None, 3, 25, 80, 129, 1, 24000.0, p, None))


def _example(n_tokens, n_frames, seed, coeff=None, speaker=0, M=80, F=129):
    rng = np.random.RandomState(seed)
    ex = {"tokens": np.concatenate([rng.randint(2, 80, n_tokens - 1), [1]]).astype(np.int32),
          "mel": rng.rand(n_frames, M).astype(np.float32) + 0.5, "linear": rng.rand(n_frames, F).astype(np.float32) + 0.5,
          "speaker_id": speaker, "name": "ex%d" % seed}
    if coeff is not None:
        ex["loss_coeff"] = coeff
    return ex


def test_prepare_batch_pads_and_rounds():
    from twvk_amd.eval_tacotron import prepare_batch
    exs = [_example(7, 11, 1, coeff=0.5, speaker=1), _example(12, 23, 2), _example(4, 20, 3, coeff=2.0, speaker=1)]
    b = prepare_batch(exs, 5)
    assert b["inputs"].shape == (3, 12) and b["inputs"].dtype == np.int32
    assert list(b["input_lengths"]) == [7, 12, 4] and list(b["n_frames"]) == [11, 23, 20]
    assert b["mel_targets"].shape == (3, 25, 80) and b["linear_targets"].shape == (3, 25, 129)      # 23 -> 25
    assert b["mel_targets"].dtype == np.float32 and b["linear_targets"].dtype == np.float32
    assert list(b["loss_coeff"]) == [0.5, 1.0, 2.0] and list(b["speaker_id"]) == [1, 0, 1]
    for i, ex in enumerate(exs):
        nt, nf = len(ex["tokens"]), len(ex["mel"])
        assert np.array_equal(b["inputs"][i, :nt], ex["tokens"]) and np.all(b["inputs"][i, nt:] == 0)
        assert np.array_equal(b["mel_targets"][i, :nf], ex["mel"]) and np.all(b["mel_targets"][i, nf:] == 0)
        assert np.array_equal(b["linear_targets"][i, :nf], ex["linear"]) and np.all(b["linear_targets"][i, nf:] == 0)
    # a longest example that is already a multiple of r is not padded further; r = 4 rounds 23 to 24
    assert prepare_batch(exs[::2], 5)["mel_targets"].shape[1] == 20
    assert prepare_batch(exs, 4)["mel_targets"].shape[1] == 24


def test_over_long_examples_are_skipped_with_a_message():
    from twvk_amd.eval_tacotron import fits, split_fitting
    assert fits(40, 8, 5) and fits(1, 8, 5) and not fits(41, 8, 5) and not fits(0, 8, 5)
    exs = [_example(5, 40, 1), _example(5, 41, 2), _example(5, 12, 3), _example(5, 300, 4)]
    said = []
    kept, skipped = split_fitting(exs, 8, 5, log=said.append)
    assert [e["name"] for e in kept] == ["ex1", "ex3"] and [e["name"] for e in skipped] == ["ex2", "ex4"]
    assert len(said) == 2 and "ex2" in said[0] and "41 frames" in said[0] and "40" in said[0]


def test_load_example_reads_the_reference_layout(tmp_path):
    from twvk_amd.eval_tacotron import load_example
    ex = _example(6, 9, 5)
    np.savez(str(tmp_path / "a.npz"), tokens=ex["tokens"], mel=ex["mel"], linear=ex["linear"])
    np.savez(str(tmp_path / "b.npz"), tokens=ex["tokens"], mel=ex["mel"], linear=ex["linear"], loss_coeff=0.25)
    a, b = load_example(str(tmp_path / "a.npz"), 0), load_example(str(tmp_path / "b.npz"), 3)
    assert a["loss_coeff"] == 1.0 and b["loss_coeff"] == 0.25 and a["speaker_id"] == 0 and b["speaker_id"] == 3
    assert a["name"] == "a" and np.array_equal(a["tokens"], ex["tokens"]) and np.array_equal(b["linear"], ex["linear"])


def test_eval_tacotron_argument_parser():
    from twvk_amd.eval_tacotron import build_parser
    p = build_parser()
    c = p.parse_args(["--load_path", "logdir", "--data_paths", "d1,d2"])
    assert c.load_path == "logdir" and c.data_paths == "d1,d2" and c.batch_size == 32
    assert c.teacher_forced is False and c.mel_out_dir is None and c.checkpoint_step is None
    c = p.parse_args(["--load_path", "l", "--data_paths", "d", "--batch_size", "4", "--teacher_forced", "--mel_out_dir", "gta"])
    assert c.batch_size == 4 and c.teacher_forced is True and c.mel_out_dir == "gta"
    for argv in (["--data_paths", "d"], ["--load_path", "l"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_add_loss_restatement_on_a_hand_made_case():
    """the checker's own add_loss against values worked out by hand (B = 1, one frame): |d| means, the band [0, 3) of 4 bins"""
    import torch_tacotron_targets_ref as TR
    mel = np.zeros((1, 1, 2), np.float32); mel_t = np.array([[[1.0, 3.0]]], np.float32)              # mean |d| = 2
    lin = np.zeros((1, 1, 4), np.float32); lin_t = np.array([[[1.0, 2.0, 4.0, 9.0]]], np.float32)     # mean 4; band bins 0..2: mean 7/3
    sr = 2 * 5000 * 4 / 3.0 - 1e-6                                   # upper = int(3.0000002) = 3, lower = int(0.099) = 0
    loss, mel_loss, linear_loss, lwc = TR.add_loss(mel, lin, mel_t, lin_t, [2.0], False, sr, 4)
    assert (loss, mel_loss, linear_loss, lwc) == (2 * 2.0 + 2 * 4.0, 2.0, 4.0, 6.0)
    loss, mel_loss, linear_loss, lwc = TR.add_loss(mel, lin, mel_t, lin_t, [2.0], True, sr, 4)
    band = (1.0 + 2.0 + 4.0) / 3.0
    assert abs(linear_loss - 0.5 * (4.0 + band)) < 1e-15 and abs(loss - (4.0 + 0.5 * 8.0 + 0.5 * 2 * band)) < 1e-14
    assert mel_loss == 2.0 and abs(lwc - (2.0 + linear_loss)) < 1e-15


def test_add_loss_refuses_outputs_that_do_not_belong_to_the_targets(model):
    """the loss kernel reads N * T_out frames of every buffer: outputs of another pass (infer overwrites them, and clears the targets) with
    the targets of an earlier, shorter one must be refused on the host"""
    import torch
    model.mel_outputs, model.linear_outputs = torch.zeros(3, 40, 80), torch.zeros(3, 40, 129)
    model.mel_targets = None                                         # the state infer leaves
    with pytest.raises(ValueError, match="forward_targets pass"):
        model.add_loss(np.zeros((3, 40, 129), np.float32))
    model.mel_targets = torch.zeros(3, 25, 80)                       # stale targets of a shorter pass
    with pytest.raises(ValueError, match="do not belong to one forward_targets pass"):
        model.add_loss(np.zeros((3, 40, 129), np.float32))
    model.mel_outputs, model.linear_outputs = torch.zeros(3, 25, 80), torch.zeros(3, 40, 129)
    with pytest.raises(ValueError, match="do not belong to one forward_targets pass"):
        model.add_loss(np.zeros((3, 25, 129), np.float32))
    model.mel_outputs = model.linear_outputs = model.mel_targets = None


class _FakeModel(object):
    """forward_targets returns targets + 1 (padding included), add_loss the batch's sizes: enough to follow evaluate()'s bookkeeping"""

    def __init__(self):
        self.calls = []

    def forward_targets(self, inputs, input_lengths, speaker_id, mel_targets, teacher_forced=False, want_linear=True, want_alignments=True):
        import torch
        self.calls.append((inputs.shape, mel_targets.shape, list(speaker_id), teacher_forced, want_linear, want_alignments))
        self.mel = torch.from_numpy(mel_targets + 1.0)
        return self.mel, None, None

    def add_loss(self, linear_targets, loss_coeff=None):
        n = float(linear_targets.shape[0])
        return {"loss": n, "mel_loss": 2 * n, "linear_loss": float(linear_targets.shape[1]), "loss_without_coeff": float(np.sum(loss_coeff))}


def test_evaluate_batches_reports_and_writes_each_mel_at_its_own_length(tmp_path):
    from twvk_amd.eval_tacotron import evaluate
    exs = [_example(7, 11, 1, coeff=0.5, speaker=1), _example(12, 23, 2), _example(4, 20, 3, coeff=2.0, speaker=1)]
    fake, said = _FakeModel(), []
    out_dir = tmp_path / "gta"
    per_batch, mean = evaluate(fake, exs, 5, batch_size=2, teacher_forced=True, mel_out_dir=str(out_dir), log=said.append)
    assert [c[0] for c in fake.calls] == [(2, 12), (1, 4)] and [c[1] for c in fake.calls] == [(2, 25, 80), (1, 20, 80)]
    assert [c[2] for c in fake.calls] == [[1, 0], [1]] and all(c[3] is True and c[4] is True for c in fake.calls)
    assert per_batch == [{"loss": 2.0, "mel_loss": 4.0, "linear_loss": 25.0, "loss_without_coeff": 1.5},
                         {"loss": 1.0, "mel_loss": 2.0, "linear_loss": 20.0, "loss_without_coeff": 2.0}]
    assert mean == {"loss": 1.5, "mel_loss": 3.0, "linear_loss": 22.5, "loss_without_coeff": 1.75}
    assert len(said) == 3 and said[0].startswith("batch 0 (2 examples, 25 frames)") and said[2].startswith("mean over 2 batches")
    assert sorted(p.name for p in out_dir.iterdir()) == ["0-ex2.npy", "1-ex1.npy", "1-ex3.npy"]
    for ex in exs:
        m = np.load(str(out_dir / ("%d-%s.npy" % (ex["speaker_id"], ex["name"]))))
        assert m.dtype == np.float32 and np.array_equal(m, ex["mel"] + 1.0)           # cut to the example's own frames
    per_batch, mean = evaluate(_FakeModel(), [], 5, log=said.append)
    assert per_batch == [] and mean == {}


def test_main_needs_a_fitting_example(tmp_path, monkeypatch):
    """main(): examples are read per directory (speaker id = index), the over-long ones dropped, and none left is an error"""
    import twvk_amd.eval_tacotron as E
    import twvk_amd.synthesizer as S

    class _Syn(object):
        def load(self, path, num_speakers=2, checkpoint_step=None):
            self.hparams, self.model, self.num_speakers = _hp(max_iters=8), _FakeModel(), num_speakers
            _Syn.last = self
    monkeypatch.setattr(S, "Synthesizer", _Syn)
    d0, d1 = tmp_path / "a", tmp_path / "b"
    d0.mkdir(); d1.mkdir()
    for d, n, seed in ((d0, 41, 1), (d1, 30, 2), (d1, 300, 3)):
        ex = _example(5, n, seed)
        np.savez(str(d / ("u%d.npz" % seed)), tokens=ex["tokens"], mel=ex["mel"], linear=ex["linear"])
    mean = E.main(["--load_path", "x", "--data_paths", "%s,%s" % (d0, d1), "--batch_size", "4"])
    assert _Syn.last.num_speakers == 2 and len(_Syn.last.model.calls) == 1
    assert _Syn.last.model.calls[0][1] == (1, 30, 80) and _Syn.last.model.calls[0][2] == [1] and _Syn.last.model.calls[0][3] is False
    assert mean["linear_loss"] == 30.0
    with pytest.raises(SystemExit, match="no example fits"):
        E.main(["--load_path", "x", "--data_paths", str(d0)])
    with pytest.raises(SystemExit, match="no \\*.npz examples"):
        E.main(["--load_path", "x", "--data_paths", str(tmp_path)])
