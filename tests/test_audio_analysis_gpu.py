"""-m gpu: waveform -> mel / linear spectrogram on the device (twv_spectrogram_analyze) against the float64 numpy checker
(tests/audio_analysis_ref.py), known answers no restatement stands behind, the general inverse (twv_inv_spectrogram), and
wav files -> npz examples -> feeder -> one training step -> generation.  Default hparams unless said; every other geometry and
kernel route is tests/test_audio_analysis_geometry_gpu.py's.

Tolerance of the float32 device path: the checker runs the SAME lines in float32; near min_level a float32 FFT's absolute error is a
large relative error, so the reachable distance depends on the signal and that run measures it.  Bar = max(8 x that distance, 1e-5):
8 x is the project's margin for another float32 order of operations (tests/test_train_gpu.py), 1e-5 is about 20 float32 spacings at
the end of the range, 4.0."""
import numpy as np
import pytest

import audio_analysis_ref as R

pytestmark = pytest.mark.gpu


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def _basis(hp):
    return R.mel_basis(hp.sample_rate, hp.fft_size, hp.num_mels)


def _bar(wav, hp, basis):
    """-> (mel64, lin64, mel bar, lin bar, mel f32 distance, lin f32 distance) for one utterance"""
    m64, l64 = R.spectrograms(wav, hp, basis)
    m32, l32 = R.spectrograms(wav, hp, basis, dtype=np.float32)
    dm, dl = np.abs(m32 - m64).max(), np.abs(l32 - l64).max()
    return m64, l64, max(8 * dm, 1e-5), max(8 * dl, 1e-5), dm, dl


def parity_report(log=print):
    """the parity measurement (also what scripts/audio_analysis_parity.py records): per utterance and output the device's distance to
    the float64 checker, the float32 checker's, and the bar.  Returns the rows."""
    from twvk_amd.audio import spectrograms
    hp = _hp()
    wavs = R.parity_signals(hp.sample_rate)
    mel, lin = spectrograms(wavs, hp)
    mel, lin = mel.cpu().numpy(), lin.cpu().numpy()
    assert mel.shape == (3, 81, hp.num_mels) and lin.shape == (3, 81, hp.num_freq)
    rows = []
    for b, wav in enumerate(wavs):
        m64, l64, bar_m, bar_l, dm, dl = _bar(wav, hp, _basis(hp))
        T = 1 + len(wav) // hp.hop_size
        assert m64.shape[0] == T
        for name, got, want, f32, bar in (("mel", mel[b, :T], m64, dm, bar_m), ("linear", lin[b, :T], l64, dl, bar_l)):
            d = np.abs(got - want).max()
            rows.append((b, len(wav), T, name, d, f32, bar))
            log("utterance %d (%d samples, %d frames) %-6s max|gpu - f64| = %.3e   max|f32 checker - f64| = %.3e   bar = %.3e"
                % (b, len(wav), T, name, d, f32, bar))
    return rows


def test_parity_ragged_batch():
    rows = parity_report()
    assert [r[2] for r in rows[::2]] == [81, 80, 26]
    for b, n, T, name, d, f32, bar in rows:
        assert d <= bar, (b, name, d, f32, bar)


def test_known_answers_silence_and_sine():
    from twvk_amd.audio import spectrograms
    hp = _hp()
    silence = np.zeros(5000, np.float32)
    mel, lin = spectrograms(silence, hp)
    assert mel.shape == (17, hp.num_mels) and lin.shape == (17, hp.num_freq)
    assert (mel.cpu().numpy() == -hp.max_abs_value).all() and (lin.cpu().numpy() == -hp.max_abs_value).all()
    mel, lin = spectrograms(silence, _hp(symmetric_mels=False))
    assert (mel.cpu().numpy() == 0.0).all() and (lin.cpu().numpy() == 0.0).all()
    # a sine at the centre of bin 200, amplitude 0.01: the periodic Hann window of `win` samples sums to win/2, so an interior frame's
    # bin holds a * win/4 times the pre-emphasis filter's gain |1 - k e^{-jw}| (exact to 1.5e-8 relative in float64: the leakage of
    # the negative-frequency image); a wrong window scale, hop or padding moves the normalised value by >= 0.05
    n, k = 12000, 200
    wav = (0.01 * np.sin(2 * np.pi * k / hp.fft_size * np.arange(n))).astype(np.float32)
    lin = spectrograms(wav, hp, mel=False)[1].cpu().numpy()
    gain = abs(1 - hp.preemphasis * np.exp(-2j * np.pi * k / hp.fft_size))
    want = R.normalize(20 * np.log10(0.01 * hp.win_size / 4 * gain) - hp.ref_level_db, 1, hp.max_abs_value, hp.min_level_db)
    for frame in (10, 20, 30):
        print("sine: linear[%d, %d] = %.6f, closed form %.6f" % (frame, k, lin[frame, k], want))
        assert abs(lin[frame, k] - want) <= 1e-4
        assert lin[frame].argmax() == k


def test_frame_counts_zero_fill_and_alone_equals_batch():
    from twvk_amd.audio import spectrograms, melspectrogram, linearspectrogram
    hp = _hp()
    wavs = R.parity_signals(hp.sample_rate)
    mel, lin = spectrograms(wavs, hp)
    for b, wav in enumerate(wavs):
        T = 1 + len(wav) // hp.hop_size
        assert (mel[b, T:] == 0).all() and (lin[b, T:] == 0).all()
        assert (lin[b, :T] != 0).any(dim=1).all()
        m1, l1 = spectrograms(wav, hp)
        assert m1.shape == (T, hp.num_mels) and l1.shape == (T, hp.num_freq)
        _, _, bar_m, bar_l, _, _ = _bar(wav, hp, _basis(hp))
        assert float((m1 - mel[b, :T]).abs().max()) <= bar_m and float((l1 - lin[b, :T]).abs().max()) <= bar_l
        assert bool((melspectrogram(wav, hp) == m1).all()) and bool((linearspectrogram(wav, hp) == l1).all())
    # (B, len) with lengths, input already on the device
    import torch
    x = torch.zeros((2, 24000), device="cuda:0")
    x[0] = torch.from_numpy(wavs[0]).cuda(); x[1, :7531] = torch.from_numpy(wavs[2]).cuda()
    m2, l2 = spectrograms(x, hp, lengths=[24000, 7531])
    _, _, bar_m, _, _, _ = _bar(wavs[0], hp, _basis(hp))
    _, _, _, bar_l, _, _ = _bar(wavs[2], hp, _basis(hp))
    assert float((m2[0] - mel[0]).abs().max()) <= bar_m and float((l2[1, :26] - lin[2, :26]).abs().max()) <= bar_l
    assert bool((l2[1, 26:] == 0).all()) and bool((m2[1, 26:] == 0).all())
    # refusals reach Python as errors
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError):
        spectrograms(np.zeros(hp.fft_size // 2, np.float32), hp)
    with pytest.raises(TwvError):
        spectrograms(x, hp, lengths=[24001, 7531])


@pytest.mark.parametrize("setting", [dict(symmetric_mels=False), dict(allow_clipping_in_normalization=False),
                                     dict(allow_clipping_in_normalization=False, symmetric_mels=False), dict(signal_normalization=False),
                                     dict(preemphasize=False), dict()])
def test_every_normalisation_against_the_checker(setting):
    from twvk_amd.audio import spectrograms
    hp = _hp(**setting)
    wav = R.noclip_signal(hp.preemphasis)          # inside [min_level_db, 0] everywhere (with pre-emphasis on): every mode accepts it
    m64, l64, bar_m, bar_l, dm, dl = _bar(wav, hp, _basis(hp))
    if hp.signal_normalization:
        scale = 1.0
    else:                                          # dB instead of [-4, 4] or [0, 4]: the same bar in units of the output's range
        scale = -hp.min_level_db / (2 * hp.max_abs_value)
        bar_m, bar_l = max(8 * dm, 1e-5 * scale), max(8 * dl, 1e-5 * scale)
    mel, lin = spectrograms(wav, hp)
    d_m, d_l = np.abs(mel.cpu().numpy() - m64).max(), np.abs(lin.cpu().numpy() - l64).max()
    print("%s: mel %.3e (f32 checker %.3e, bar %.3e)  linear %.3e (f32 checker %.3e, bar %.3e)" % (setting, d_m, dm, bar_m, d_l, dl, bar_l))
    assert d_m <= bar_m and d_l <= bar_l


@pytest.mark.parametrize("symmetric", [True, False])
def test_no_clip_modes_raise_where_the_reference_asserts(symmetric):
    from twvk_amd.audio import spectrograms, melspectrogram
    hp = _hp(allow_clipping_in_normalization=False, symmetric_mels=symmetric)
    basis = _basis(hp)
    quiet = np.zeros(5000, np.float32)                                             # S = -120 dB < min_level_db
    loud = (0.9 * np.sin(2 * np.pi * 200 / hp.fft_size * np.arange(6000))).astype(np.float32)      # a bin at +28 dB > 0
    for wav in (quiet, loud):
        assert R.spectrograms(wav, hp, basis) == (None, None)                      # the checker's (= the reference's) assertion fires
        with pytest.raises(AssertionError):
            spectrograms(wav, hp)
        with pytest.raises(AssertionError):
            melspectrogram(wav, hp)
    spectrograms(R.noclip_signal(hp.preemphasis), hp)                               # and does not fire here


def _inverse_case(hp, channels, lo, hi, seed):
    rng = np.random.RandomState(seed)
    B, T = 2, 14
    spec = rng.uniform(lo, hi, (B, T, channels)).astype(np.float32)
    u = rng.rand(B, T, hp.num_freq).astype(np.float32)
    return spec, u


@pytest.mark.parametrize("setting,lo,hi", [(dict(symmetric_mels=False), -0.5, 4.5),
                                           (dict(allow_clipping_in_normalization=False), -4.5, 4.5),
                                           (dict(allow_clipping_in_normalization=False, symmetric_mels=False), -0.5, 4.5),
                                           (dict(signal_normalization=False), -110.0, 5.0),
                                           (dict(preemphasize=False), -4.5, 4.5)])
def test_inv_linear_spectrogram_other_normalisations(setting, lo, hi):
    from twvk_amd.audio import inv_linear_spectrogram
    hp = _hp(griffin_lim_iters=3, **setting)
    spec, u = _inverse_case(hp, hp.num_freq, lo, hi, seed=11)
    got = inv_linear_spectrogram(spec, hp, uniforms=u).cpu().numpy()
    want = np.stack([R.inv_spectrogram(spec[b], u[b], hp, 3) for b in range(2)])
    assert got.shape == want.shape
    # tests/test_audio_gpu.py's form: per utterance, 8 x the float32 run of the checker (floor 1e-6 of the peak), never above 2e-4
    import griffin_lim_cases as G
    for b in range(2):
        e_gpu, e_f32 = G.rel(got[b], want[b]), G.rel(R.inv_spectrogram_f32(spec[b], u[b], hp, 3), want[b])
        print(setting, "utterance %d: e_gpu %.3e  e_f32 %.3e" % (b, e_gpu, e_f32))
        assert e_gpu <= min(G.bar(e_f32), 2e-4), (b, e_gpu, e_f32)


def test_default_normalisation_is_the_same_through_both_fronts():
    """twv_inv_spectrogram(norm_mode 1) and twv_inv_linear_spectrogram share the loop and the arithmetic: identical samples"""
    import ctypes as C
    import torch
    from twvk_amd import _lib
    from twvk_amd.audio import inv_linear_spectrogram, _ptr
    hp = _hp(griffin_lim_iters=2)
    spec, u = _inverse_case(hp, hp.num_freq, -4.5, 4.5, seed=2)
    a = inv_linear_spectrogram(spec, hp, uniforms=u)
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_griffin_lim_create(hp.fft_size, hp.hop_size, hp.win_size, 14, 2, C.byref(h)))
    ws = torch.empty(L.twv_griffin_lim_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device="cuda:0")
    out = torch.empty((2, L.twv_griffin_lim_samples(h)), dtype=torch.float32, device="cuda:0")
    s, uu = torch.from_numpy(spec).cuda(), torch.from_numpy(u).cuda()
    _lib.check(L.twv_inv_spectrogram(h, _ptr(s), hp.num_freq, None, _ptr(uu), 2, hp.power, hp.ref_level_db, hp.max_abs_value, hp.min_level_db, 1,
                                     hp.preemphasis, _ptr(ws), _ptr(out), None))
    torch.cuda.synchronize()
    L.twv_griffin_lim_destroy(h)
    assert torch.equal(a, out)


@pytest.mark.parametrize("iters", [0, 3])
def test_inv_mel_spectrogram_matches_numpy(iters):
    """Bar: 8 x the distance of the restatement with its front (denormalise, dB -> amplitude, inverse basis, ** power) in float32, with
    the linear path's 2e-4 of the peak as its floor -- and never above 8 x the distance of the WHOLE path run in float32
    (audio_analysis_ref.inv_spectrogram_f32; floor 1e-6 of the peak), the bar of tests/test_audio_gpu.py."""
    from twvk_amd.audio import inv_mel_spectrogram, mel_basis
    hp = _hp(griffin_lim_iters=iters)
    spec, u = _inverse_case(hp, hp.num_mels, -4.5, 4.5, seed=5 + iters)
    basis = mel_basis(hp)
    inv = np.linalg.pinv(basis.astype(np.float64)).astype(np.float32)
    got = inv_mel_spectrogram(spec, hp, uniforms=u).cpu().numpy()
    assert got.shape == (2, hp.hop_size * 13)
    for b in range(2):
        y64 = R.inv_spectrogram(spec[b], u[b], hp, iters, inv)
        y32 = R.inv_spectrogram(spec[b], u[b], hp, iters, inv, dtype=np.float32)
        peak = np.abs(y64).max()
        f32 = np.abs(y32 - y64).max() / peak
        rel = np.abs(got[b] - y64).max() / peak
        import griffin_lim_cases as G
        whole = G.rel(R.inv_spectrogram_f32(spec[b], u[b], hp, iters, inv), y64)
        print("inv_mel iters %d utterance %d: max|gpu - f64| / peak = %.3e, float32 front %.3e, whole float32 run %.3e" % (iters, b, rel, f32, whole))
        assert rel <= min(max(8 * f32, 2e-4), G.bar(whole))


def test_wavs_to_examples_to_training_step_and_generation(tmp_path):
    """through every layer: wav files -> preprocess.main -> npz -> DataFeederWavenet -> WaveNetTrainer.step; mel -> WaveNetModel.generate"""
    import torch
    from scipy.io import wavfile
    from helpers import make_model, mol_uniforms
    from twvk_amd import weights as W
    from twvk_amd import preprocess
    from twvk_amd.train import WaveNetTrainer
    from twvk_amd.train_vocoder import DataFeederWavenet
    hp = _hp()
    rng = np.random.RandomState(8)
    sr = hp.sample_rate
    t = np.arange(2 * sr) / sr
    (tmp_path / "wav").mkdir()
    for i in range(4):
        env = np.clip(np.sin(np.pi * t / 2.0) * 3, 0, 1)                                   # quiet at both ends: the trim has work to do
        x = env * (0.4 * np.sin(2 * np.pi * (110 + 40 * i) * t) + 0.05 * rng.randn(len(t)))
        if i == 0:
            wavfile.write(str(tmp_path / "wav" / "u0.wav"), sr, x.astype(np.float32))
        else:
            wavfile.write(str(tmp_path / "wav" / ("u%d.wav" % i)), sr, np.clip(x * 32767, -32768, 32767).astype(np.int16))
    lines = []
    r = preprocess.main(["--in_dir", str(tmp_path / "wav"), "--out_dir", str(tmp_path / "data"), "--batch_size", "3"], log=lines.append)
    assert len(r["written"]) == 4 and not r["skipped"]
    for p in r["written"]:
        d = np.load(p)
        assert sorted(d.files) == ["audio", "linear", "mel", "mel_frames", "time_steps"]
        T = int(d["mel_frames"])
        assert d["mel"].shape == (T, hp.num_mels) and d["linear"].shape == (T, hp.num_freq) and d["audio"].shape == (T * hp.hop_size,)
        assert int(d["time_steps"]) == T * hp.hop_size and 100 < T <= 161 and np.abs(d["audio"]).max() <= 1.0
        assert np.isfinite(d["mel"]).all() and d["mel"].min() >= -hp.max_abs_value and d["mel"].max() <= hp.max_abs_value
        assert d["mel"].max() > 0, "a 0.4-amplitude tone must reach the upper half of the range"
    with pytest.raises(ValueError, match="u9.wav"):
        wavfile.write(str(tmp_path / "u9.wav"), 16000, np.zeros(4000, np.int16))
        preprocess.read_wav(str(tmp_path / "u9.wav"), sr)
    # feeder -> one training step on a small model
    dil = [1, 2, 4, 8, 1, 2, 4, 8]
    hp_small = _hp(sample_size=1200)
    B = 2
    feeder = DataFeederWavenet([str(tmp_path / "data")], B, receptive_field=64, hp=hp_small)
    np.random.seed(4)
    audio, lc, gc = feeder.next_batch()
    assert audio.shape == (B, 1200) and lc.shape == (B, 4, hp.num_mels) and gc.shape == (B,)
    tensors = W.random_tensors(W.tensor_specs(len(dil), S=64, use_biases=True, upsample_factor=(5, 5, 12)), seed=0, scale=0.05)
    net = make_model(B, dil, tensors, S=64)
    tr = WaveNetTrainer(net, sample_size=1200)
    tr.load_weights(tensors)
    loss = float(tr.step(audio, lc, gc).item())
    assert np.isfinite(loss)
    # the mel of one utterance as local conditioning of the generation path
    gen = make_model(1, dil, tensors, S=64)
    mel = np.load(r["written"][1])["mel"][None, :2]
    up = gen.create_upsample(torch.from_numpy(mel).cuda())
    out = gen.generate(up[:, :600].contiguous(), [0], np.zeros(1, np.float32), mol_uniforms(1, 600, 10))
    out = out.cpu().numpy()
    assert out.shape[-1] == 600 and np.isfinite(out).all()
