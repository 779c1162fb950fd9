"""-m gpu: the attention types other than bah_mon_norm (tacotron.py:127-144) on the split decoder kernel (tc_decoder_g_kernel's AK_*
instantiations) against the float64 restatement tests/torch_attention_ref.py, and their launch-geometry / placement invariants."""
import numpy as np
import pytest

from helpers import first_mismatch

pytestmark = pytest.mark.gpu

TYPES = ["bah_mon", "bah_norm", "bah", "luong", "luong_scaled", "loc_sen"]
SOFTMAX = [t for t in TYPES if t != "bah_mon"]
# float32 kernel vs float64 restatement: max |kernel - restatement| / max |restatement| per output.  Measured on the MI355X over the
# cases below: 0.9e-7 .. 3.1e-7 for mel, linear and alignments everywhere except loc_sen at 200 steps (mel 9.7e-7, alignments 1.03e-5:
# the cumulative state carries the rounding of every earlier step into the location features).  The bound is 5x the largest of these;
# a wrong mask, bias, tap or scale moves these outputs by 1e-3 or more.
RTOL = 5e-5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _tokens(N, T, lengths, seed):
    rng = np.random.RandomState(seed)
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    for n, ln in enumerate(lengths):
        tok[n, ln - 1] = 1                      # EOS
        tok[n, ln:] = 0                         # pad
    return tok, np.asarray(lengths, np.int32)


def _model(hp, num_speakers, seed):
    import torch_attention_ref as AR
    from twvk_amd.tacotron import Tacotron
    m = Tacotron(hp, num_speakers=num_speakers)
    w = AR.random_tensors(m.specs, seed)
    m.load_weights(w)
    return m, w


def _rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def _against_restatement(m, w, hp, num_speakers, tok, ln, spk, attention_type):
    import torch_attention_ref as AR
    mel, lin, al = [x.cpu().numpy() for x in m.infer(tok, ln, spk)]
    mel_r, lin_r, al_r = AR.infer(w, AR.Dims(hp, num_speakers), tok, ln, spk, attention_type)
    d = (_rel(mel, mel_r), _rel(lin, lin_r), _rel(al, al_r))
    print("%s N=%d T=%d steps=%d: rel distance mel %.2e linear %.2e alignments %.2e" % ((attention_type,) + tok.shape + (hp.max_iters,) + d))
    assert d[0] <= RTOL and d[1] <= RTOL and d[2] <= RTOL, (attention_type, d)
    assert np.all(al[np.arange(tok.shape[1])[None, :] >= ln[:, None]] == 0)          # nothing attends past input_lengths
    return mel, lin, al


@pytest.mark.parametrize("attention_type", TYPES)
@pytest.mark.parametrize("geometry", ["small", "default"])
def test_attention_type_against_the_restatement(torch_cuda, attention_type, geometry):
    if geometry == "small":
        hp = _hp(max_iters=6, enc_bank_size=4, post_bank_size=3, num_freq=129, attention_type=attention_type)
        N, T, lengths = 3, 19, [19, 12, 7]
    else:
        hp = _hp(max_iters=25, attention_type=attention_type)
        N, T, lengths = 3, 40, [40, 29, 13]
    m, w = _model(hp, 2, seed=61)
    tok, ln = _tokens(N, T, lengths, 62)
    spk = np.array([1, 0, 1], np.int32)
    assert m.decoder_kernel_name(N, T) == "tc_decoder_g_kernel"
    mel, lin, al = _against_restatement(m, w, hp, 2, tok, ln, spk, attention_type)
    if attention_type in SOFTMAX:                # the softmax alignments sum to one over the valid positions
        for n in range(N):
            assert np.abs(al[n, :ln[n]].astype(np.float64).sum(axis=0) - 1.0).max() <= 1e-5, (n, al[n, :ln[n]].sum(axis=0))


@pytest.mark.parametrize("attention_type", ["bah", "loc_sen"])
def test_attention_type_200_steps(torch_cuda, attention_type):
    """the full decode (200 steps = 1000 mel frames): loc_sen's cumulative state runs over every step"""
    hp = _hp(max_iters=200, attention_type=attention_type)
    m, w = _model(hp, 2, seed=71)
    tok, ln = _tokens(3, 40, [40, 31, 9], 72)
    _, _, al = _against_restatement(m, w, hp, 2, tok, ln, np.array([0, 1, 1], np.int32), attention_type)
    if attention_type == "loc_sen":              # the emitted alignments are the per-step ones (they sum to 1), not the cumulative state
        assert np.abs(al[0].astype(np.float64).sum(axis=0) - 1.0).max() <= 1e-5


@pytest.mark.parametrize("attention_type", TYPES)
def test_decoder_groups_do_not_change_results(torch_cuda, attention_type):
    """1, 4, 8, 16 workgroups per utterance and the library's own choice: the same bits; a second pass reuses the exchange buffers"""
    hp = _hp(max_iters=7, enc_bank_size=3, post_bank_size=2, num_freq=65, attention_type=attention_type)
    m, _ = _model(hp, 2, seed=81)
    tok, ln = _tokens(3, 37, [37, 20, 5], 82)
    spk = np.array([0, 1, 0], np.int32)
    ref = None
    for groups in (0, 1, 4, 8, 16):
        m.set_option("decoder_groups", groups)
        for _ in range(2):
            out = [x.cpu().numpy() for x in m.infer(tok, ln, spk)]
            if ref is None:
                ref = out
            for name, a, b in zip(("mel", "linear", "alignments"), out, ref):
                assert first_mismatch(a, b) is None, (groups, name, first_mismatch(a, b))


@pytest.mark.parametrize("attention_type", TYPES)
def test_resident_and_single_workgroup_kernels_refuse(torch_cuda, attention_type):
    from twvk_amd._lib import TwvError
    hp = _hp(max_iters=3, enc_bank_size=2, post_bank_size=2, num_freq=33, attention_type=attention_type)
    m, _ = _model(hp, 2, seed=91)
    tok, ln = _tokens(2, 11, [11, 4], 92)
    for groups in (32, -1):
        m.set_option("decoder_groups", groups)
        assert m.decoder_kernel_name(2, 11) == ""
        with pytest.raises(TwvError, match="split decoder"):
            m.infer(tok, ln, np.array([0, 1], np.int32))


@pytest.mark.parametrize("attention_type", TYPES)
def test_an_utterance_does_not_depend_on_its_place_in_the_batch(torch_cuda, attention_type):
    """BASELINE configs[2]'s size (B = 32, 101 tokens, 200 steps), no checker: an utterance's outputs are the same bits wherever it sits
    in the batch and whoever sits next to it (split decoder at 8 workgroups per utterance; the batch of five runs at 16)"""
    hp = _hp(attention_type=attention_type)
    m, _ = _model(hp, 2, seed=3)
    rng = np.random.RandomState(3)
    N, T = 32, 101
    lengths = np.array([T - (i * 7) % 60 for i in range(N)], np.int32)
    tok, _ = _tokens(N, T, lengths, 4)
    spk = (np.arange(N) % 2).astype(np.int32)
    mel, lin, al = [x.cpu().numpy() for x in m.infer(tok, lengths, spk)]
    assert np.isfinite(mel).all() and mel.shape == (N, 1000, 80)
    perm = rng.permutation(N)
    mel_p, lin_p, al_p = [x.cpu().numpy() for x in m.infer(tok[perm], lengths[perm], spk[perm])]
    assert first_mismatch(mel_p, mel[perm]) is None and first_mismatch(lin_p, lin[perm]) is None and first_mismatch(al_p, al[perm]) is None
    sub = np.array([17, 3, 30, 8, 21])
    mel_s, lin_s, al_s = [x.cpu().numpy() for x in m.infer(tok[sub], lengths[sub], spk[sub])]
    assert first_mismatch(mel_s, mel[sub]) is None and first_mismatch(lin_s, lin[sub]) is None and first_mismatch(al_s, al[sub]) is None
    if attention_type in SOFTMAX:
        for n in range(N):
            assert np.abs(al[n, :lengths[n]].astype(np.float64).sum(axis=0) - 1.0).max() <= 1e-5
            assert np.all(al[n, lengths[n]:] == 0)


def test_loc_sen_checkpoint_round_trip(torch_cuda, tmp_path):
    """a loc_sen checkpoint (TF-V2 bundle + params.json) through Synthesizer.load and synthesize: the names tacotron_specs emits
    are the whole interface (checkpoint.restore_variables unchanged); the restored model computes the bits of the one it was saved from"""
    from twvk_amd import checkpoint as ckpt
    from twvk_amd.hparams import save_hparams
    from twvk_amd.synthesizer import Synthesizer
    hp = _hp(max_iters=6, griffin_lim_iters=2, attention_type="loc_sen")
    m, w = _model(hp, 2, seed=101)
    logdir = tmp_path / "logdir"; logdir.mkdir()
    save_hparams(str(logdir), hp)
    ckpt.write_bundle(str(logdir / "model.ckpt-2000"), ckpt.tacotron_variables(w))
    syn = Synthesizer()
    syn.load(str(logdir), num_speakers=2, hparams=_hp())                # attention_type comes from params.json
    assert syn.hparams.attention_type == "loc_sen"
    toks = [[5, 9, 33, 12, 1], [7, 7, 1]]
    out = syn.infer(toks, speaker_ids=[1, 0])
    tok = np.array([[5, 9, 33, 12, 1], [7, 7, 1, 0, 0]], np.int32)
    mel, lin, al = m.infer(tok, np.array([5, 3], np.int32), np.array([1, 0], np.int32))
    assert first_mismatch(out["mel"].cpu().numpy(), mel.cpu().numpy()) is None
    assert first_mismatch(out["alignments"].cpu().numpy(), al.cpu().numpy()) is None
    wavs = tmp_path / "wavs"; wavs.mkdir()
    # (untrimmed: with random weights the attention reaches the last input within a step or two, and the trimmed spectrogram would be
    # shorter than Griffin-Lim's reflect padding)
    res = syn.synthesize(tokens=toks, base_path=str(wavs), speaker_ids=[1, 0], attention_trim=False, seed=3)
    assert res == [True, True] and len(list(wavs.glob("*.wav"))) == 2 and len(list(wavs.glob("*.npy"))) == 2


@pytest.mark.parametrize("groups", [0, 4])
def test_model_type_simple_with_bah(torch_cuda, groups):
    """model_type 'simple' (the speaker embedding concatenated inside the decoder) x BahdanauAttention: against the restatement"""
    hp = _hp(max_iters=5, enc_bank_size=3, post_bank_size=2, num_freq=65, model_type="simple", attention_type="bah")
    m, w = _model(hp, 4, seed=111)
    assert dict(m.specs)["decoder/attention_wrapper/gru_cell/gates/kernel"] == (128 + 16 + 256 + 256, 512)
    m.set_option("decoder_groups", groups)
    tok, ln = _tokens(5, 41, [41, 30, 17, 8, 2], 112)
    _against_restatement(m, w, hp, 4, tok, ln, np.array([3, 0, 1, 2, 3], np.int32), "bah")
