"""-m gpu: Tacotron passes with caller-supplied alignments (twv_tacotron_infer_manual: tc_decoder_g_kernel's AK_MAN instantiations and
tc_decoder_kernel<false, true>), the alignment edit kernel, and Synthesizer.synthesize_manual.

Two exact properties carry most of the weight: a pass fed its own alignments reproduces its bits (the context stage and everything
behind it are the code of the mechanisms' passes), and tensors that only a mechanism reads cannot influence a manual pass at all.
Shapes are those of tests/test_attention_types_gpu.py: "small" (T = 19, not a multiple of 4) and "groups" (T = 37)."""
import numpy as np
import pytest

from helpers import first_mismatch
from test_attention_types_gpu import RTOL, _hp, _model, _rel, _tokens        # the bar and the cases of the attention types' own tests

pytestmark = pytest.mark.gpu

ALL_TYPES = ["bah_mon_norm", "bah_mon", "bah_norm", "bah", "luong", "luong_scaled", "loc_sen"]
SMALL = dict(max_iters=6, enc_bank_size=4, post_bank_size=3, num_freq=129)
GROUPS = dict(max_iters=7, enc_bank_size=3, post_bank_size=2, num_freq=65)
NAMES = ("mel", "linear", "alignments")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def _np(out):
    return [x.cpu().numpy() for x in out]


def _same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        assert a.shape == b.shape and first_mismatch(a, b) is None, (what, name, a.shape, b.shape, first_mismatch(a, b))


def _random_alignments(N, steps, T, lengths, seed):
    """non-negative rows that sum to 1 over the valid positions, and small non-zero values past the lengths"""
    rng = np.random.RandomState(seed)
    man = np.zeros((N, steps, T), np.float32)
    for n, ln in enumerate(lengths):
        a = rng.rand(steps, ln) ** 4
        man[n, :, :ln] = a / a.sum(axis=1, keepdims=True)
        man[n, :, ln:] = 1e-3 * (0.5 + rng.rand(steps, T - ln))
    return man


@pytest.mark.parametrize("case", ALL_TYPES + ["simple"])
def test_a_pass_fed_its_own_alignments_reproduces_its_bits(torch_cuda, case):
    """infer at its default route, then infer_manual(edit_alignments(alignments, 0)): mel, linear and alignments bit for bit; the same at
    3 < max_iters steps and at one step against forward_targets(teacher_forced=False).  model_type 'simple' also on the single-workgroup
    kernel, which serves it for manual passes only."""
    simple = case == "simple"
    hp = _hp(model_type="simple", **SMALL) if simple else _hp(attention_type=case, **SMALL)
    speakers = 4 if simple else 2
    m, _ = _model(hp, speakers, seed=61)
    tok, ln = _tokens(3, 19, [19, 12, 7], 62)
    spk = np.array([3, 0, 2], np.int32) if simple else np.array([1, 0, 1], np.int32)
    first = m.infer(tok, ln, spk)
    man = m.edit_alignments(first[2], 0)
    assert tuple(man.shape) == (3, 6, 19)
    want = _np(first)
    assert m.manual_kernel_name(3, 19) == "tc_decoder_g_kernel"
    _same(_np(m.infer_manual(tok, ln, spk, man)), want, case)
    if simple:
        m.set_option("decoder_groups", -1)
        assert m.manual_kernel_name(3, 19) == "tc_decoder_kernel"
        _same(_np(m.infer_manual(tok, ln, spk, man)), want, "simple on tc_decoder_kernel")
        m.set_option("decoder_groups", 0)
    for steps in (3, 1):
        targets = np.zeros((3, steps * hp.reduction_factor, hp.num_mels), np.float32)
        free = m.forward_targets(tok, ln, spk, targets, teacher_forced=False)
        assert tuple(free[2].shape) == (3, 19, steps)
        short = _np(m.infer_manual(tok, ln, spk, m.edit_alignments(free[2], 0)))
        assert short[0].shape == (3, steps * hp.reduction_factor, hp.num_mels) and short[1].shape == (3, steps * hp.reduction_factor, hp.num_freq)
        _same(short, _np(free), (case, steps))
        assert first_mismatch(short[0], want[0][:, :steps * hp.reduction_factor]) is None      # (and a free-running prefix of the long pass)


@pytest.mark.parametrize("attention_type", ["bah_mon_norm", "bah", "luong_scaled", "loc_sen"])
def test_the_mechanism_cannot_leak_into_a_manual_pass(torch_cuda, attention_type):
    """every tensor that only the mechanism reads -- the memory layer and what _attention_specs lists: query layer, attention_v / _g / _b,
    the score bias, loc_sen's filters, layer, variable and bias -- filled with NaN and repacked: the manual pass is finite and bit for bit
    the clean model's"""
    from twvk_amd.tacotron import _attention_specs
    hp = _hp(attention_type=attention_type, **SMALL)
    m, w = _model(hp, 2, seed=63)
    tok, ln = _tokens(3, 19, [19, 12, 7], 64)
    spk = np.array([0, 1, 1], np.int32)
    man = _random_alignments(3, 6, 19, ln, 65)
    clean = _np(m.infer_manual(tok, ln, spk, man))
    assert all(np.isfinite(x).all() for x in clean)
    only = ["memory_layer/kernel"] + [n for n, _ in _attention_specs(hp)]
    assert len(only) == {"bah_mon_norm": 6, "bah": 3, "luong_scaled": 2, "loc_sen": 7}[attention_type]
    poisoned = dict(w)
    for name in only:
        poisoned[name] = np.full_like(w[name], np.nan)
    m.load_weights(poisoned)
    assert bool(torch_cuda.isnan(m._packed).any())                         # (the poison is in the packed weights the kernels read)
    got = _np(m.infer_manual(tok, ln, spk, man))
    assert all(np.isfinite(x).all() for x in got)
    _same(got, clean, attention_type)


@pytest.mark.parametrize("attention_type", ["bah_mon_norm", "loc_sen"])
def test_manual_pass_against_the_float64_checker(torch_cuda, attention_type):
    """random alignments, non-zero past the lengths, two speakers: max |kernel - checker| / max |checker| of mel and linear within the
    bar of the attention types' own tests (the same graph with a harder attention in front); the emitted alignments are the manual
    values bit for bit, past the lengths too.  Measured on the MI355X: see profiles/tacotron_manual_attention_parity.txt."""
    import torch_attention_ref as AR
    import torch_manual_attention_ref as MR
    hp = _hp(attention_type=attention_type, **SMALL)
    m, w = _model(hp, 2, seed=66)
    tok, ln = _tokens(3, 19, [19, 12, 7], 67)
    spk = np.array([1, 0, 1], np.int32)
    man = _random_alignments(3, 6, 19, ln, 68)
    assert np.all(man[1, :, 12:] > 0) and np.abs(man[2, :, :7].astype(np.float64).sum(axis=1) - 1).max() < 1e-6
    mel, lin, al = _np(m.infer_manual(tok, ln, spk, man))
    mel_r, lin_r, al_r = MR.infer_manual(w, AR.Dims(hp, 2), tok, ln, spk, man)
    d = (_rel(mel, mel_r), _rel(lin, lin_r))
    print("manual %s N=3 T=19 steps=6: rel distance mel %.2e linear %.2e (bar %.0e)" % (attention_type, d[0], d[1], RTOL))
    assert d[0] <= RTOL and d[1] <= RTOL, (attention_type, d)
    assert first_mismatch(al, man.transpose(0, 2, 1)) is None and np.array_equal(al_r, man.transpose(0, 2, 1).astype(np.float64))


def test_launch_geometry_does_not_change_a_manual_pass(torch_cuda):
    """1 .. 16 workgroups per utterance, the library's choice and the single-workgroup kernel, on one XCD or spread, prenet and query
    stage split or whole: the same bits, twice each (the second pass reuses the exchange buffers).  decoder_groups = 32 is refused, and
    the handle serves `infer` afterwards as before."""
    from twvk_amd._lib import TwvError
    hp = _hp(**GROUPS)
    m, _ = _model(hp, 2, seed=81)
    tok, ln = _tokens(3, 37, [37, 20, 5], 82)
    spk = np.array([0, 1, 0], np.int32)
    man = _random_alignments(3, 7, 37, ln, 83)
    infer_kernel = m.decoder_kernel_name(3, 37)
    plain = _np(m.infer(tok, ln, spk))
    settings = [(g, loc, -1) for g in (0, 1, 4, 8, 16, -1) for loc in (0, 1)] + [(8, 1, 0), (8, 1, 1), (8, 0, 0), (8, 0, 1)]
    ref = None
    for groups, local, split_all in settings:
        m.set_option("decoder_groups", groups); m.set_option("decoder_local", local); m.set_option("decoder_split_all", split_all)
        assert m.manual_kernel_name(3, 37) == ("tc_decoder_kernel" if groups == -1 else "tc_decoder_g_kernel")
        for _ in range(2):
            out = _np(m.infer_manual(tok, ln, spk, man))
            ref = ref or out
            _same(out, ref, (groups, local, split_all))
    m.set_option("decoder_local", 1); m.set_option("decoder_split_all", -1)
    m.set_option("decoder_groups", 32)
    assert m.manual_kernel_name(3, 37) == ""
    with pytest.raises(TwvError, match="XCD-local decoder kernel takes no caller-supplied alignments"):
        m.infer_manual(tok, ln, spk, man)
    m.set_option("decoder_groups", 0)
    assert m.decoder_kernel_name(3, 37) == infer_kernel
    _same(_np(m.infer(tok, ln, spk)), plain, "infer after the refusal")
    assert first_mismatch(ref[0], plain[0]) is not None                # (the manual pass was a different pass)


def test_causality_and_independence(torch_cuda):
    """the rows of step 4 reach the frames of step 4 and none before; an utterance does not depend on its neighbours"""
    hp = _hp(**SMALL)
    m, _ = _model(hp, 2, seed=84)
    tok, ln = _tokens(3, 19, [19, 12, 7], 85)
    spk = np.array([1, 1, 0], np.int32)
    man = _random_alignments(3, 6, 19, ln, 86)
    base = _np(m.infer_manual(tok, ln, spk, man))
    other = man.copy()
    other[:, 4] = _random_alignments(3, 1, 19, ln, 87)[:, 0]
    moved = _np(m.infer_manual(tok, ln, spk, other))
    r = hp.reduction_factor
    assert first_mismatch(moved[0][:, :4 * r], base[0][:, :4 * r]) is None
    for n in range(3):
        assert first_mismatch(moved[0][n, 4 * r:5 * r], base[0][n, 4 * r:5 * r]) is not None, n
    assert first_mismatch(moved[2][:, :, :4], base[2][:, :, :4]) is None and first_mismatch(moved[2][:, :, 5:], base[2][:, :, 5:]) is None
    for n in range(3):
        alone = _np(m.infer_manual(tok[n:n + 1], ln[n:n + 1], spk[n:n + 1], man[n:n + 1]))
        _same(alone, [x[n:n + 1] for x in base], ("alone", n))


def _planted(B, T, steps, seed):
    """alignments with the ties an argmax can meet: all-zero rows, a maximum that occurs twice, a maximum at the last step"""
    rng = np.random.RandomState(seed)
    a = rng.rand(B, T, steps).astype(np.float32)
    for b in range(B):
        a[b, b % T] = 0.0                                              # all-zero row: argmax 0
        a[b, T - 1] = 0.0                                              # (the last row as well: a padded row of a real pass)
        if T > 2:
            a[b, 1, steps - 1] = 2.0                                   # the maximum at the last step
        if T > 3 and steps > 2:
            a[b, 2, [steps // 3, steps - 1 - steps // 4]] = 3.0        # the maximum twice: the first wins
        if T > 4 and steps > 70:
            a[b, 3, [5, 69]] = 4.0                                     # ... in different 64-step rounds of the row scan
            a[b, 4, [70, 6]] = 5.0
    return a


@pytest.mark.parametrize("shape", [(3, 19, 6), (2, 70, 200), (1, 5, 1), (2, 33, 65)])
def test_edit_kernel_against_the_numpy_restatement(torch_cuda, shape):
    """modes 0-3, bit for bit, into NaN-filled buffers (every element is written): T_in below, at and above the 32-row tile, steps below
    and above the 64 lanes of the row scan and the 32-step tile, one step"""
    import ctypes as C
    from twvk_amd import _lib
    from twvk_amd.tacotron import alignment_edit_numpy
    B, T, steps = shape
    a = _planted(B, T, steps, 90 + T)
    dev = torch_cuda.from_numpy(a).cuda()
    for mode in range(4):
        out = torch_cuda.full((B, steps, T), float("nan"), dtype=torch_cuda.float32, device="cuda")
        _lib.check(_lib.lib().twv_tacotron_alignment_edit(C.c_void_p(dev.data_ptr()), B, T, steps, mode, C.c_void_p(out.data_ptr()),
                                                          C.c_void_p(torch_cuda.cuda.current_stream().cuda_stream)))
        got = out.cpu().numpy()
        assert first_mismatch(got, alignment_edit_numpy(a, mode)) is None, (shape, mode, first_mismatch(got, alignment_edit_numpy(a, mode)))
        if mode in (1, 3):
            assert np.array_equal((got == 1.0).sum(axis=1) >= 1, np.ones((B, T), bool))      # every encoder row got its 1
    assert first_mismatch(dev.cpu().numpy(), a) is None                 # the input is left alone


def test_edit_kernel_on_a_real_pass(torch_cuda):
    from twvk_amd.tacotron import alignment_edit_numpy
    hp = _hp(**GROUPS)
    m, _ = _model(hp, 2, seed=81)
    tok, ln = _tokens(3, 37, [37, 20, 5], 82)
    al = m.infer(tok, ln, np.array([0, 1, 0], np.int32))[2]
    host = al.cpu().numpy()
    assert np.all(host[2, 5:] == 0)
    for mode in range(4):
        got = m.edit_alignments(al, mode)
        assert tuple(got.shape) == (3, 7, 37)
        assert first_mismatch(got.cpu().numpy(), alignment_edit_numpy(host, mode)) is None, mode
        assert first_mismatch(m.edit_alignments(host, mode).cpu().numpy(), got.cpu().numpy()) is None      # an array goes the same way
    assert np.all(m.edit_alignments(al, 1).cpu().numpy()[2, 0, 5:] == 1)     # padded rows: all zero, so their 1 sits at step 0


def test_synthesize_manual(torch_cuda, oracle, tmp_path):
    """synthesizer.py:165-198 as two passes: the plain pass's files, then `.manual` files from the pass fed the edited alignments; a
    base_alignment_path pass over the first pass's saved alignments gives the first pass's wav; the CLI's --base_alignment_path reaches the
    same code"""
    import io
    from scipy.io import wavfile
    from twvk_amd import checkpoint as ckpt
    from twvk_amd.audio import inv_linear_spectrogram
    from twvk_amd.e2e import attention_trim_frames
    from twvk_amd.hparams import save_hparams
    from twvk_amd.ops import wav_to_int16
    from twvk_amd.synthesizer import Synthesizer, main as synth_main
    hp = _hp(max_iters=6, griffin_lim_iters=3)
    d = oracle.taco_dims(max_iters=6, num_freq=hp.num_freq)
    tensors = oracle.taco_random_tensors(d, seed=5)
    syn = Synthesizer()
    syn.load(tensors, num_speakers=2, hparams=hp)
    toks = [[5, 9, 33, 12, 1], [7, 7, 1]]
    both = tmp_path / "both"
    res = syn.synthesize_manual(tokens=toks, base_path=str(both), speaker_ids=[1, 0], manual_attention_mode=1, seed=11)
    assert res == ([True, True], [True, True])
    wavs = sorted(str(p) for p in both.glob("*.wav"))
    manual = [w for w in wavs if w.endswith(".manual.wav")]
    plain = [w for w in wavs if not w.endswith(".manual.wav")]
    assert len(manual) == 2 and len(plain) == 2 and [w.replace(".wav", ".manual.wav") for w in plain] == manual
    assert sorted(str(p) for p in both.glob("*.npy")) == sorted(w.replace(".wav", ".npy") for w in wavs)
    out = syn.infer(toks, speaker_ids=[1, 0])
    mel2, lin2, al2 = syn.model.infer_manual(out["sequences"], out["input_lengths"], [1, 0], syn.model.edit_alignments(out["alignments"], 1))
    for i in range(2):
        for path, (mel, lin, al) in ((plain[i], (out["mel"], out["linear"], out["alignments"])), (manual[i], (mel2, lin2, al2))):
            n = attention_trim_frames(al[i].cpu().numpy(), len(out["sequences"][i]), hp.reduction_factor)      # trimmed by its own alignments
            want = inv_linear_spectrogram(lin[i:i + 1, :n], hp, seed=11)
            sr, data = wavfile.read(path)
            assert sr == hp.sample_rate and np.array_equal(data, wav_to_int16(want).cpu().numpy().reshape(-1)), path
            assert first_mismatch(np.load(path.replace(".wav", ".npy")), mel[i, :n].cpu().numpy()) is None
    # saved alignments (synthesizer.py:265-267 writes "<base_path>/<idx>.npy", (T_in, steps)) fed back through base_alignment_path
    saved = tmp_path / "saved"; saved.mkdir()
    for i in range(2):
        np.save(str(saved / ("%d.npy" % i)), out["alignments"][i].cpu().numpy(), allow_pickle=False)
    first = syn.synthesize(tokens=toks, speaker_ids=[1, 0], seed=11)
    again = syn.synthesize_manual(tokens=toks, speaker_ids=[1, 0], base_alignment_path=str(saved) + "/", seed=11)
    assert isinstance(first[0], bytes) and again == first
    assert wavfile.read(io.BytesIO(again[1]))[0] == hp.sample_rate
    given = syn.synthesize_manual(tokens=toks, speaker_ids=[1, 0], manual_alignments=[out["alignments"][0].cpu().numpy(), out["alignments"][1].cpu().numpy()[:3]],
                                  seed=11)                             # (the second utterance's rows up to its own length: padded with zeros)
    assert given == first
    with pytest.raises(ValueError):
        syn.synthesize_manual(tokens=toks)                             # nothing manual asked for
    with pytest.raises(ValueError):
        syn.synthesize(tokens=toks, base_alignment_path=str(saved) + "/")
    # the CLI
    logdir = tmp_path / "logdir"; logdir.mkdir()
    save_hparams(str(logdir), hp)
    ckpt.write_bundle(str(logdir / "model.ckpt-1000"), ckpt.tacotron_variables(tensors))
    cli2 = tmp_path / "cli2"
    assert synth_main(["--load_path", str(logdir), "--sample_path", str(cli2), "--tokens", "5,9,33,12,1", "--num_speakers", "2",
                       "--speaker_id", "1", "--seed", "11", "--base_alignment_path", str(saved) + "/"]) is True
    got2 = sorted(str(p) for p in cli2.glob("*.wav"))
    assert len(got2) == 1 and np.array_equal(wavfile.read(got2[0])[1], wavfile.read(plain[0])[1])
