"""-m "not gpu": caller-supplied alignments (tacotron.py:122-123, rnn_wrappers.py:369-374) and the alignment edits (synthesizer.py:165-190)
at the host surface -- the C entries and what they refuse before any device is looked at, the numpy restatement of the four edit modes
against hand-written answers, and the float64 checker tests/torch_manual_attention_ref.py anchored to tests/torch_attention_ref.py."""
import ctypes as C
import os

import numpy as np
import pytest

INVALID, UNSUPPORTED = 1, 2            # include/twv_amd.h TWV_E_*


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _model(num_speakers=2, **kw):
    from twvk_amd.tacotron import Tacotron
    return Tacotron(_hp(**kw), num_speakers=num_speakers, device="cpu")


class _Call(object):
    """twv_tacotron_infer_manual with every argument acceptable -- host words stand in for the device buffers: a refusal comes before any
    of them is read -- and single arguments replaced"""

    def __init__(self, m):
        self.m = m
        self.word = (C.c_int32 * 4)()
        p = C.cast(self.word, C.c_void_p)
        self.args = dict(h=m._h, packed=p, tokens=p, lengths=p, speaker_ids=p, batch=2, t_in=7, manual=p, steps=3, workspace=p, mel=p,
                         linear=None, alignments=None, status=p, stream=None)

    def __call__(self, **kw):
        a = dict(self.args, **kw)
        return self.m._L.twv_tacotron_infer_manual(a["h"], a["packed"], a["tokens"], a["lengths"], a["speaker_ids"], a["batch"], a["t_in"],
                                                   a["manual"], a["steps"], a["workspace"], a["mel"], a["linear"], a["alignments"],
                                                   a["status"], a["stream"])


def test_the_new_entries_are_exported_and_declared():
    from twvk_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "twv_amd.h")).read()
    for name in ("twv_tacotron_infer_manual", "twv_tacotron_manual_kernel_name", "twv_tacotron_alignment_edit"):
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in header, name
    assert "rnn_wrappers.py:369-374" in header and "synthesizer.py:165-190" in header      # the reference lines, as the other entries cite theirs


def test_infer_manual_refuses_before_the_device_is_looked_at():
    from twvk_amd import _lib
    m = _model(max_iters=6)
    call = _Call(m)
    assert call(h=None) == INVALID
    for name in ("packed", "tokens", "lengths", "manual", "workspace", "mel", "status"):
        assert call(**{name: None}) == INVALID, name
        assert b"null" in _lib.lib().twv_last_error()
    for steps in (0, -1, 7):
        assert call(steps=steps) == INVALID, steps
        assert b"max_iters" in _lib.lib().twv_last_error()
    for batch in (0, -3):
        assert call(batch=batch) == INVALID, batch
    for t_in in (0, -1, 1025):
        assert call(t_in=t_in) == INVALID, t_in
    assert call(speaker_ids=None) == INVALID                       # a two-speaker model
    assert b"speaker_ids" in _lib.lib().twv_last_error()
    # the XCD-local kernel takes no manual alignments: refused for the option alone, with a message that says so
    m.set_option("decoder_groups", 32)
    assert call() == UNSUPPORTED
    msg = _lib.lib().twv_last_error().decode()
    assert "decoder_groups = 32" in msg and "caller-supplied alignments" in msg
    assert m.manual_kernel_name(2, 7) == ""


def test_manual_kernel_name_needs_no_device():
    """a manual pass is served by the split kernel at 0, 1, ..., 16 workgroups per utterance and by the single-workgroup kernel at -1, for
    every attention type and for model_type 'simple' -- where `infer` refuses -1"""
    for kw, speakers in ((dict(), 2), (dict(attention_type="loc_sen"), 2), (dict(attention_type="luong"), 1), (dict(model_type="simple"), 3)):
        m = _model(speakers, **kw)
        for groups in (0, 1, 2, 4, 8, 16):
            m.set_option("decoder_groups", groups)
            assert m.manual_kernel_name(3, 19) == "tc_decoder_g_kernel", (kw, groups)
        m.set_option("decoder_groups", -1)
        assert m.manual_kernel_name(3, 19) == "tc_decoder_kernel", kw
        assert m.manual_kernel_name(0, 19) == "" and m.manual_kernel_name(3, 0) == ""
    assert m._L.twv_tacotron_manual_kernel_name(None, 3, 19) == b""


def test_alignment_edit_refuses_before_the_device_is_looked_at():
    from twvk_amd import _lib
    L = _lib.lib()
    word = (C.c_float * 4)()
    p = C.cast(word, C.c_void_p)
    assert L.twv_tacotron_alignment_edit(None, 1, 2, 2, 0, p, None) == INVALID
    assert L.twv_tacotron_alignment_edit(p, 1, 2, 2, 0, None, None) == INVALID
    for batch, t_in, steps in ((0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2), (1, -2, 2), (1, 2, -2)):
        assert L.twv_tacotron_alignment_edit(p, batch, t_in, steps, 0, p, None) == INVALID, (batch, t_in, steps)
    for mode in (-1, 4, 17):
        assert L.twv_tacotron_alignment_edit(p, 1, 2, 2, mode, p, None) == INVALID, mode
        assert b"mode" in L.twv_last_error()


def test_alignment_edit_numpy_known_answers():
    from twvk_amd.tacotron import alignment_edit_numpy
    # one utterance, four encoder rows over three steps: a plain maximum in the middle, an all-zero row (argmax 0), a maximum that
    # occurs twice (the first wins), a maximum at the last step
    a = np.array([[[0.25, 0.5, 0.125],
                   [0.0, 0.0, 0.0],
                   [0.5, 0.125, 0.5],
                   [0.125, 0.25, 0.75]]], np.float32)
    t = np.array([[[0.25, 0.0, 0.5, 0.125],
                   [0.5, 0.0, 0.125, 0.25],
                   [0.125, 0.0, 0.5, 0.75]]], np.float32)
    want = {0: t,
            1: np.array([[[0, 1, 1, 0], [1, 0, 0, 0], [0, 0, 0, 1]]], np.float32),
            2: np.array([[[0.0625, 0.0, 0.25, 0.015625], [0.25, 0.0, 0.015625, 0.0625], [0.015625, 0.0, 0.25, 0.5625]]], np.float32),
            3: np.array([[[0.25, 1.0, 1.0, 0.125], [1.0, 0.0, 0.125, 0.25], [0.125, 0.0, 0.5, 1.0]]], np.float32)}
    for mode in range(4):
        got = alignment_edit_numpy(a, mode)
        assert got.dtype == np.float32 and got.shape == (1, 3, 4) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, want[mode]), (mode, got)
    assert np.array_equal(a, np.array([[[0.25, 0.5, 0.125], [0, 0, 0], [0.5, 0.125, 0.5], [0.125, 0.25, 0.75]]], np.float32))    # the input is left alone
    # steps = 1: every row's argmax is step 0
    b = np.array([[[0.5], [0.0], [-2.0]], [[3.0], [0.25], [0.0]]], np.float32)
    assert np.array_equal(alignment_edit_numpy(b, 0), b.transpose(0, 2, 1))
    assert np.array_equal(alignment_edit_numpy(b, 1), np.ones((2, 1, 3), np.float32))
    assert np.array_equal(alignment_edit_numpy(b, 2), np.array([[[0.25, 0.0, 4.0]], [[9.0, 0.0625, 0.0]]], np.float32))
    assert np.array_equal(alignment_edit_numpy(b, 3), np.ones((2, 1, 3), np.float32))
    assert np.array_equal(b, np.array([[[0.5], [0.0], [-2.0]], [[3.0], [0.25], [0.0]]], np.float32))     # (one step: the transpose is no copy by itself)
    # the utterances of a batch are edited each by its own argmax
    c = np.array([[[0.0, 1.0]], [[1.0, 0.0]]], np.float32)
    assert np.array_equal(alignment_edit_numpy(c, 1), np.array([[[0.0], [1.0]], [[1.0], [0.0]]], np.float32))
    for bad in (4, -1, None):
        with pytest.raises(ValueError):
            alignment_edit_numpy(a, bad)
    with pytest.raises(ValueError):
        alignment_edit_numpy(a[0], 0)


@pytest.mark.parametrize("num_speakers", [1, 2])
def test_checker_fed_a_pass_its_own_alignments_gives_that_pass(num_speakers):
    """torch_manual_attention_ref.infer_manual(alignments of torch_attention_ref.infer) == torch_attention_ref.infer, float64 bit for bit;
    with other alignments the outputs move, and the emitted alignments are always the given ones"""
    import torch_attention_ref as AR
    import torch_manual_attention_ref as MR
    from twvk_amd.tacotron import tacotron_specs
    hp = _hp(max_iters=6, enc_bank_size=4, post_bank_size=3, num_freq=129)
    w = AR.random_tensors(tacotron_specs(hp, num_speakers), 11)
    rng = np.random.RandomState(12)
    N, T, lengths = 3, 19, [19, 12, 7]
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    for n, ln in enumerate(lengths):
        tok[n, ln - 1] = 1
        tok[n, ln:] = 0
    spk = np.array([1, 0, 1], np.int32) if num_speakers > 1 else None
    dims = AR.Dims(hp, num_speakers)
    mel, lin, al = AR.infer(w, dims, tok, np.asarray(lengths), spk, "bah_mon_norm")
    got = MR.infer_manual(w, dims, tok, np.asarray(lengths), spk, al.transpose(0, 2, 1))
    for name, x, y in zip(("mel", "linear", "alignments"), got, (mel, lin, al)):
        assert x.dtype == np.float64 and x.shape == y.shape and np.array_equal(x, y), name
    assert AR._Mechanism.__name__ == "_Mechanism"                  # (the checker puts the mechanism back)
    # no attention tensor is read: the same bits without them
    bare = {k: v for k, v in w.items() if "bahdanau_monotonic_attention" not in k}
    assert len(bare) == len(w) - 5
    again = MR.infer_manual(bare, dims, tok, np.asarray(lengths), spk, al.transpose(0, 2, 1))
    assert all(np.array_equal(x, y) for x, y in zip(again, got))
    # three steps of other alignments, non-zero past the lengths: used as given
    man = rng.rand(N, 3, T)
    mel3, lin3, al3 = MR.infer_manual(w, dims, tok, np.asarray(lengths), spk, man)
    assert mel3.shape == (N, 3 * hp.reduction_factor, hp.num_mels) and lin3.shape == (N, 3 * hp.reduction_factor, hp.num_freq)
    assert np.array_equal(al3, man.transpose(0, 2, 1))
    assert np.array_equal(mel3[:, :hp.reduction_factor], MR.infer_manual(w, dims, tok, np.asarray(lengths), spk, man[:, :1])[0])
    assert np.abs(mel3 - mel[:, :3 * hp.reduction_factor]).max() > 1e-3
