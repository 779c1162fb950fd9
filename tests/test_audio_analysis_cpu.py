"""No GPU: the waveform -> spectrogram feature's surface, its checker against the reference's own numpy functions (fixtures made by
tests/golden/make_reference_numpy_audio.py), the mel basis, the C-ABI's argument refusals and the host half of preprocess.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_analysis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("twv_spectrogram_create", "twv_spectrogram_destroy", "twv_spectrogram_frames", "twv_spectrogram_workspace_bytes",
                    "twv_spectrogram_analyze", "twv_inv_spectrogram")


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


def test_entry_points_exist():
    """fails without the feature: the C-ABI names (header, binding, library) and the Python functions"""
    from twvk_amd import _lib, audio
    hdr = open(os.path.join(ROOT, "include", "twv_amd.h")).read()
    declared = set(re.findall(r"\b(twv_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in ("melspectrogram", "linearspectrogram", "spectrograms", "inv_mel_spectrogram", "mel_basis"):
        assert callable(getattr(audio, name)), name
    from twvk_amd import preprocess
    assert callable(preprocess.main) and callable(preprocess.assemble_example)


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_numpy_audio.npz"))


def test_checker_equals_the_reference_functions():
    """float64 against float64, the same expressions: 1e-12"""
    g = _golden()
    k, min_db, max_abs = float(g["preemphasis_k"]), float(g["min_level_db"]), float(g["max_abs_value"])
    assert np.abs(R.preemphasis(g["wav"], k) - g["preemphasis"]).max() <= 1e-12
    assert np.array_equal(g["preemphasis_off"], g["wav"])
    assert np.abs(R.amp_to_db(g["amp"], min_db) - g["amp_to_db"]).max() <= 1e-12
    assert R.amp_to_db(g["amp"], min_db).min() == pytest.approx(min_db, abs=1e-12)            # the floor at min_level was reached
    from oracle import audio_np as A
    assert np.abs(A.db_to_amp(g["db"]) / g["db_to_amp"] - 1).max() <= 1e-12
    assert int(g["pad_lr"]) == 1024
    for mode in (1, 2, 3, 4):
        S = g["S_wide"] if mode in (1, 2) else g["S_in"]
        want = g["normalize_%d" % mode]
        assert np.abs(R.normalize(S, mode, max_abs, min_db) - want).max() <= 1e-12, mode
        if mode in (1, 2):                                                                        # both clip edges were reached
            assert want.max() == max_abs and want.min() == (-max_abs if mode == 1 else 0.0)
        else:
            assert float(g["normalize_%d_asserts_on_wide" % mode]) == 1.0
            with pytest.raises(AssertionError):
                R.normalize(g["S_wide"], mode, max_abs, min_db)
        assert np.abs(R.denormalize(g["D_wide"], mode, max_abs, min_db) - g["denormalize_%d" % mode]).max() <= 1e-12, mode


def test_mel_basis_properties_and_checker_agreement():
    from twvk_amd.audio import mel_basis
    hp = _hp()
    b = mel_basis(hp)
    assert b.shape == (80, 1025) and b.dtype == np.float32
    assert (b >= 0).all()
    for i, row in enumerate(b):
        nz = np.flatnonzero(row)
        assert nz.size and nz[-1] - nz[0] + 1 == nz.size, "filter %d is not one contiguous run" % i
    assert (b != 0).sum(axis=0).max() <= 2
    area = b.astype(np.float64).sum(axis=1) * hp.sample_rate / hp.fft_size
    assert np.abs(area - 1).max() <= 0.02, (area.min(), area.max())
    want = R.mel_basis(hp.sample_rate, hp.fft_size, hp.num_mels)
    assert np.abs(b - want).max() <= 1e-6, np.abs(b - want).max()


def _create(L, n_fft, hop, win, n_mels, basis, max_samples, batch):
    h = C.c_void_p()
    rc = L.twv_spectrogram_create(n_fft, hop, win, n_mels, basis.ctypes.data_as(C.c_void_p) if basis is not None else None, max_samples, batch,
                                  C.byref(h))
    return rc, h


def test_spectrogram_create_refusals_without_a_device():
    from twvk_amd import _lib
    L = _lib.lib()
    basis = np.ones((4, 129), np.float32)
    rc, h = _create(L, 256, 64, 200, 4, basis, 1000, 2)
    assert rc == 0 and L.twv_spectrogram_frames(h) == 1 + 1000 // 64 and L.twv_spectrogram_workspace_bytes(h) > 2 * 16 * (256 * 4 + 129 * 8)
    L.twv_spectrogram_destroy(h)
    rc, h = _create(L, 256, 64, 200, 0, None, 1000, 1)                    # no mel output wanted: no basis needed
    assert rc == 0
    L.twv_spectrogram_destroy(h)
    for args, what in [((255, 64, 200, 4, basis, 1000, 2), "odd n_fft"),
                       ((256, 64, 257, 4, basis, 1000, 2), "win_length > n_fft"),
                       ((256, 64, 200, 4, None, 1000, 2), "n_mels > 0 without a basis"),
                       ((256, 64, 200, 4, basis, 128, 2), "max_samples <= n_fft/2"),
                       ((256, 0, 200, 4, basis, 1000, 2), "hop < 1"),
                       ((256, 64, 200, 4, basis, 1000, 0), "batch < 1")]:
        rc, h = _create(L, *args)
        assert rc == 1, what                                                # TWV_E_INVALID
        assert L.twv_last_error()
    # analyze checks the lengths before it touches the device
    rc, h = _create(L, 256, 64, 200, 4, basis, 1000, 2)
    assert rc == 0
    ws = C.create_string_buffer(16)                                         # never reached
    for lengths, what in [([1000, 128], "len <= n_fft/2"), ([1001, 500], "len > max_samples")]:
        arr = np.asarray(lengths, np.int32)
        rc = L.twv_spectrogram_analyze(h, C.cast(ws, C.c_void_p), arr.ctypes.data_as(C.c_void_p), 0.97, 20.0, -100.0, 4.0, 1, C.cast(ws, C.c_void_p),
                                       C.cast(ws, C.c_void_p), None, None, None)
        assert rc == 1, what
    L.twv_spectrogram_destroy(h)


def test_n_fft_8192_is_refused_before_any_device_work():
    """the magnitude tile of sa_output_kernel is 4 x (n_fft/2 + 1) floats: 65 536 bytes at n_fft 8190, the largest accepted, 65 552 at
    8192.  analyze refuses on the host (TWV_E_UNSUPPORTED): the pointers are never touched and nothing is launched -- this test has no
    device.  (8190 itself runs in tests/test_audio_analysis_geometry_gpu.py.)"""
    from twvk_amd import _lib
    L = _lib.lib()
    rc, h = _create(L, 8192, 2048, 8192, 0, None, 9000, 1)
    assert rc == 0
    ws = C.create_string_buffer(16)                                         # never reached
    rc = L.twv_spectrogram_analyze(h, C.cast(ws, C.c_void_p), None, 0.97, 20.0, -100.0, 4.0, 1, C.cast(ws, C.c_void_p), None, C.cast(ws, C.c_void_p),
                                   None, None)
    assert rc == 2 and b"n_fft above 8190" in L.twv_last_error()
    L.twv_spectrogram_destroy(h)
    rc, h = _create(L, 8190, 2048, 8190, 0, None, 9000, 1)
    assert rc == 0
    L.twv_spectrogram_destroy(h)


def test_geometry_table_conditions_hold_on_the_checker():
    """tests/audio_analysis_cases.py's table, on the checker alone, so that a change of the inputs cannot empty a case of the GPU tests:
    the amplitude bar stays tight (e_f32 <= 2.5e-6: twice the worst measured, 1.2e-6), no float64 linear value sits on a clip edge and
    no mel value on the upper one (there the amplitude measure would be blind), at most half of an utterance's mel values sit on the
    lower one (worst: 0.40, the row with ten empty filters), and the float64 run's own agreement with oracle.audio_np.stft
    (audio_analysis_ref.stages) holds at every row.  Also what the rows are there for."""
    import audio_analysis_cases as K
    from test_audio_analysis_gpu import _bar
    assert len(K.TABLE) == len(K.SEEDS) == 10
    assert sorted(r[0] for r in K.TABLE if r[0] % 4 == 2) == [126, 2058, 8190]
    assert K.empty_filters(K.TABLE[5]) == 10 and K.empty_filters(K.TABLE[9]) == 1 and K.n_mels_of(K.TABLE[9]) == 300
    band = np.flatnonzero(K.basis(K.TABLE[9])[100])
    assert band[0] == 200 and band[-1] == 259 and (K.basis(K.TABLE[9])[[0, 299]] != 0).all()
    assert 4 * 4 * (8190 // 2 + 1) == 64 * 1024 and 4 * 8190 == 32760 and 2058 // 2 + 1 == 1024 + 6
    for row in K.TABLE:
        hp, basis, wavs, refs = K.row_case(row)                             # (the float64 run asserts against oracle.audio_np.stft)
        assert all(len(w) > row[0] // 2 and w.dtype == np.float32 for w in wavs) and basis.dtype == np.float32
        for b, (w, ref) in enumerate(zip(wavs, refs)):
            m64, l64, m32, l32 = ref
            assert m64.shape == (1 + len(w) // row[2], K.n_mels_of(row)) and l64.shape == (m64.shape[0], row[0] // 2 + 1)
            assert m32.dtype == l32.dtype == np.float32
            for name, d, d32, bar, e, e32, abar in K.measures(m32, l32, ref, hp):
                assert e == e32 and 0 < e32 <= 2.5e-6 and abar <= K.AMP_BAR_CAP, (K.row_id(row), b, name, e32, abar)
            assert not (np.abs(l64) == hp.max_abs_value).any(), (K.row_id(row), b)
            assert not (m64 == hp.max_abs_value).any(), (K.row_id(row), b)
            assert (m64 == -hp.max_abs_value).mean() <= 0.5, (K.row_id(row), b)
    # the dB bar is test_audio_analysis_gpu._bar's, unchanged
    hp, basis, wavs, refs = K.row_case(K.TABLE[6])
    _, _, bar_m, bar_l, dm, dl = _bar(wavs[0], hp, basis)
    assert (bar_m, dm) == K.db_bar(refs[0][2], refs[0][0]) and (bar_l, dl) == K.db_bar(refs[0][3], refs[0][1])
    # the inputs of the no-clip settings at (126, 100, 30): accepted, and refused
    for setting in (dict(allow_clipping_in_normalization=False), dict(allow_clipping_in_normalization=False, symmetric_mels=False)):
        hp = K.hparams(K.SETTINGS_ROW, **setting)
        m, l = R.spectrograms(R.noclip_signal(hp.preemphasis), hp, basis)
        assert m is not None and l is not None
        assert R.spectrograms(np.zeros(500, np.float32), hp, basis) == (None, None)


def test_trim_on_a_built_signal():
    """0.5 s of zeros, 1 s of tone, 0.5 s of zeros at 24 kHz: the kept interval contains the whole tone and at most trim_fft_size samples
    of silence on either side"""
    from twvk_amd.preprocess import trim_indices, trim_silence
    hp = _hp()
    sr = hp.sample_rate
    t = np.arange(sr) / sr
    wav = np.concatenate([np.zeros(sr // 2), 0.5 * np.sin(2 * np.pi * 440 * t), np.zeros(sr // 2)]).astype(np.float32)
    start, end = trim_indices(wav, hp.trim_top_db, hp.trim_fft_size, hp.trim_hop_size)
    print("trim: start %d samples before the tone, end %d after" % (sr // 2 - start, end - (sr // 2 + sr)))
    assert 0 <= sr // 2 - start <= hp.trim_fft_size
    assert 0 <= end - (sr // 2 + sr) <= hp.trim_fft_size
    assert np.array_equal(trim_silence(wav, hp), wav[start:end])
    assert trim_indices(np.zeros(4000), hp.trim_top_db, hp.trim_fft_size, hp.trim_hop_size) == (0, 4000)   # all frames equal the maximum


def test_example_assembly_with_an_injected_mel():
    from twvk_amd.preprocess import assemble_example, prepare_wav
    from twvk_amd.train_vocoder import crop_example
    hp = _hp(trim_silence=False)
    rng = np.random.RandomState(3)
    wav = prepare_wav(rng.uniform(-0.3, 0.3, 24017), hp)
    assert np.abs(wav).max() == pytest.approx(hp.rescaling_max, rel=1e-6)
    frames = 1 + len(wav) // hp.hop_size
    mel = rng.uniform(-4, 4, (frames, hp.num_mels)).astype(np.float32)
    lin = rng.uniform(-4, 4, (frames, hp.num_freq)).astype(np.float32)
    ex = assemble_example(wav, mel, lin, hp)
    assert sorted(ex) == ["audio", "linear", "mel", "mel_frames", "time_steps"]
    assert ex["mel_frames"] == frames and ex["time_steps"] == len(ex["audio"]) == frames * hp.hop_size
    assert ex["audio"].dtype == np.float32 and np.array_equal(ex["audio"], np.pad(wav, hp.fft_size // 2, "reflect")[:frames * hp.hop_size])
    a, m = crop_example(ex["audio"], ex["mel"], 50, hp.hop_size, randint=lambda lo, hi: hi - 1)
    assert a.shape == (50 * hp.hop_size,) and m.shape == (50, hp.num_mels)
    # the skip rule of datasets/moon.py:116-117
    assert assemble_example(wav, mel, lin, _hp(max_mel_frames=frames - 1)) is None
    assert assemble_example(wav, mel, lin, _hp(max_mel_frames=frames - 1, clip_mels_length=False)) is not None
    with pytest.raises(NotImplementedError):
        prepare_wav(wav, _hp(input_type="mulaw-quantize"))


def test_checker_float32_switch_stays_float32():
    """the tolerance yardstick of the GPU tests: the same lines in float32 give float32 results close to, and different from, float64"""
    hp = _hp()
    rng = np.random.RandomState(0)
    wav = rng.uniform(-0.3, 0.3, 3000)
    basis = R.mel_basis(hp.sample_rate, hp.fft_size, hp.num_mels)
    m64, l64 = R.spectrograms(wav, hp, basis)
    m32, l32 = R.spectrograms(wav, hp, basis, dtype=np.float32)
    assert m64.shape == (11, 80) and l64.shape == (11, 1025)
    assert m32.dtype == l32.dtype == np.float32 and m64.dtype == np.float64
    assert 0 < np.abs(l32 - l64).max() < 1e-3 and 0 < np.abs(m32 - m64).max() < 1e-4
