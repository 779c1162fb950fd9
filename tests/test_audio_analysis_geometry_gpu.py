"""-m gpu: twv_spectrogram_analyze at every geometry and kernel route of tests/audio_analysis_cases.py's table -- both instantiations
of sa_frame_kernel, FFT lengths that are no power of two, nbin below 256 and a little above 1024, the LDS limit (n_fft 8190), empty
filters, a dense basis, n_mels > 256 -- against the float64 numpy checker, in two measures that must both hold: the dB bar of
tests/test_audio_analysis_gpu.py and the amplitude-domain bar (audio_analysis_cases: e <= max(8 x e_f32, 1e-6) of the largest
amplitude, uniform over the bins).  The measured device distances are recorded by scripts/audio_analysis_parity.py in
profiles/audio_analysis_parity.txt, not here."""
import ctypes as C
import functools

import numpy as np
import pytest

import audio_analysis_cases as K
import audio_analysis_ref as R

pytestmark = pytest.mark.gpu

ROW_IDS = [K.row_id(r) for r in K.TABLE]


@functools.lru_cache(maxsize=None)
def _device_batch(row):
    """the ragged batch of a row through the Python front, once: (mel, linear) host arrays, read-only"""
    from twvk_amd.audio import spectrograms
    hp, basis, wavs, _ = K.row_case(row)
    mel, lin = spectrograms(list(wavs), hp, mel_basis=basis)
    mel, lin = mel.cpu().numpy(), lin.cpu().numpy()
    mel.setflags(write=False); lin.setflags(write=False)
    return mel, lin


def _frames(n, hop):
    return 1 + n // hop


def _hold(rows, what):
    for name, d, d32, bar, e, e32, abar in rows:
        print("%s %-6s max|gpu - f64| = %.3e (f32 checker %.3e, bar %.3e)   e = %.3e (e_f32 %.3e, bar %.3e)" % (what, name, d, d32, bar, e, e32, abar))
        assert d <= bar, (what, name, "dB", d, d32, bar)
        assert e <= abar, (what, name, "amplitude", e, e32, abar)


def parity_report(log=print):
    """per (row, utterance, output): the device's distance, the float32 checker's and the bar, in both measures
    (scripts/audio_analysis_parity.py records it)"""
    out = []
    for row in K.TABLE:
        hp, basis, wavs, refs = K.row_case(row)
        mel, lin = _device_batch(row)
        for b, (w, ref) in enumerate(zip(wavs, refs)):
            T = _frames(len(w), hp.hop_size)
            for name, d, d32, bar, e, e32, abar in K.measures(mel[b, :T], lin[b, :T], ref, hp):
                out.append((row, b, name, d, d32, bar, e, e32, abar))
                log("%-26s utterance %d (%4d samples, %2d frames) %-6s dB: gpu %.3e  f32 %.3e  bar %.3e   amplitude: e %.3e  e_f32 %.3e  bar %.3e"
                    % (K.row_id(row), b, len(w), T, name, d, d32, bar, e, e32, abar))
    return out


@pytest.mark.parametrize("row", K.TABLE, ids=ROW_IDS)
def test_parity_ragged_batch(row):
    hp, basis, wavs, refs = K.row_case(row)
    mel, lin = _device_batch(row)
    assert mel.shape == (3, _frames(max(row[4]), hp.hop_size), K.n_mels_of(row)) and lin.shape == (3, mel.shape[1], row[0] // 2 + 1)
    for b, (w, ref) in enumerate(zip(wavs, refs)):
        T = _frames(len(w), hp.hop_size)
        assert ref[0].shape[0] == T
        _hold(K.measures(mel[b, :T], lin[b, :T], ref, hp), "%s utterance %d" % (K.row_id(row), b))
        assert not mel[b, T:].any() and not lin[b, T:].any(), "rows past an utterance's frames are exactly 0"


@pytest.mark.parametrize("row", K.ALONE_ROWS, ids=[K.row_id(r) for r in K.ALONE_ROWS])
def test_alone_against_batch(row):
    """each utterance run alone (another max_samples, frames and batch in the handle) within the bars of its rows in the batch"""
    from twvk_amd.audio import spectrograms
    hp, basis, wavs, refs = K.row_case(row)
    mel, lin = _device_batch(row)
    for b, (w, ref) in enumerate(zip(wavs, refs)):
        T = _frames(len(w), hp.hop_size)
        m1, l1 = spectrograms(np.array(w), hp, mel_basis=basis)              # (a writable copy: the cached signals are read-only)
        assert m1.shape == (T, K.n_mels_of(row)) and l1.shape == (T, row[0] // 2 + 1)
        # the batch's rows stand where the float64 checker stood: the same two measures, the same bars
        for name, got, other, x64, x32 in (("mel", m1.cpu().numpy(), mel[b, :T], ref[0], ref[2]), ("linear", l1.cpu().numpy(), lin[b, :T], ref[1], ref[3])):
            bar, _ = K.db_bar(x32, x64)
            abar = K.amp_bar(K.amp_rel(x32, x64, hp))
            d = float(np.abs(got - other).max())
            e = float(np.abs(K.amplitude(got, hp) - K.amplitude(other, hp)).max() / K.amplitude(x64, hp).max())
            print("%s utterance %d %-6s alone against batch: %.3e (bar %.3e)   e %.3e (bar %.3e)" % (K.row_id(row), b, name, d, bar, e, abar))
            assert d <= bar and e <= abar, (b, name, d, bar, e, abar)


@pytest.mark.parametrize("row", K.ONE_OUTPUT_ROWS, ids=[K.row_id(r) for r in K.ONE_OUTPUT_ROWS])
def test_one_output_requested_equals_both(row):
    """mel=False / linear=False take the kernel's lin_out == NULL / mel_out == NULL branches: the same bits as the both-outputs call"""
    from twvk_amd.audio import spectrograms
    hp, basis, wavs, _ = K.row_case(row)
    mel, lin = _device_batch(row)
    only_lin = spectrograms(list(wavs), hp, mel_basis=basis, mel=False)
    only_mel = spectrograms(list(wavs), hp, mel_basis=basis, linear=False)
    assert only_lin[0] is None and only_mel[1] is None
    assert np.array_equal(only_lin[1].cpu().numpy(), lin) and np.array_equal(only_mel[0].cpu().numpy(), mel)


NOCLIP = (dict(allow_clipping_in_normalization=False), dict(allow_clipping_in_normalization=False, symmetric_mels=False))


@pytest.mark.parametrize("setting", [dict(signal_normalization=False), dict(symmetric_mels=False), dict(preemphasize=False)] + list(NOCLIP),
                         ids=["no-normalisation", "asymmetric", "no-preemphasis", "no-clip", "no-clip-asymmetric"])
def test_normalisations_and_preemphasis_off_the_default_geometry(setting):
    """(126, 100, 30): nbin 64, so one wave of sa_output_kernel holds every bin and three hold none (their min / max stay +-inf and
    must not reach the atomics).  The clipping settings take the row's batch; the no-clip settings take an input the reference's
    assertion accepts (every S inside [min_level_db, 0]: the negative branch of both atomics) and two it refuses (silence, S = -120;
    a loud tone, S > 0: the positive branch of the max), which raise AssertionError on the device path too."""
    from twvk_amd.audio import spectrograms
    row = K.SETTINGS_ROW
    hp, basis = K.hparams(row, **setting), K.basis(row)
    if hp.signal_normalization:
        floor = 1e-5
    else:                                          # dB instead of [-4, 4]: test_audio_analysis_gpu's floor in units of the output's range
        floor = 1e-5 * -hp.min_level_db / (2 * hp.max_abs_value)
    if setting in NOCLIP:
        wavs = [R.noclip_signal(hp.preemphasis)]
    else:
        wavs = list(K.signals(row))
    refs = [K.checkers(w, hp, basis, key=(row, i, tuple(sorted(setting.items())))) for i, w in enumerate(wavs)]
    assert all(r[0] is not None and r[1] is not None for r in refs), "the reference's assertion must not fire on this input"
    mel, lin = spectrograms(wavs, hp, mel_basis=basis)
    mel, lin = mel.cpu().numpy(), lin.cpu().numpy()
    for b, (w, ref) in enumerate(zip(wavs, refs)):
        T = _frames(len(w), hp.hop_size)
        _hold(K.measures(mel[b, :T], lin[b, :T], ref, hp, floor), "%s utterance %d" % (setting, b))
        assert not mel[b, T:].any() and not lin[b, T:].any()
    if setting in NOCLIP:
        quiet = np.zeros(500, np.float32)
        loud = (0.9 * np.sin(2 * np.pi * 20 / row[0] * np.arange(600))).astype(np.float32)       # bin 20 holds 0.9 * win / 4 * 0.94 = 21: +6 dB
        for w in (quiet, loud):
            assert R.spectrograms(w, hp, basis) == (None, None)
            with pytest.raises(AssertionError):
                spectrograms(w, hp, mel_basis=basis)
            with pytest.raises(AssertionError):
                spectrograms(w, hp, mel_basis=basis, linear=False)


def test_n_fft_8192_is_refused_and_8190_is_the_last_accepted():
    """8190 runs (the table's row); 8192 would need 65 552 bytes for the magnitude tile: TWV_E_UNSUPPORTED through the Python front
    (tests/test_audio_analysis_cpu.py shows on the host that nothing is launched)"""
    from twvk_amd._lib import TwvError
    from twvk_amd.audio import spectrograms
    row = (8192, 8192, 2048, 80, (9000,))
    with pytest.raises(TwvError, match=r"twv_amd error 2: .*n_fft above 8190"):
        spectrograms(np.zeros(9000, np.float32), K.hparams(row), mel_basis=np.zeros((80, 4097), np.float32))
    assert _device_batch(K.TABLE[8])[1].shape == (3, 5, 4096)


@pytest.mark.parametrize("row", K.STALE_ROWS, ids=[K.row_id(r) for r in K.STALE_ROWS])
def test_nothing_stale_nothing_behind(row):
    """the C-ABI itself: the workspace holds NaN before the first call, both outputs hold NaN with 1024 marked floats behind each.
    Afterwards every output element is finite (no live or dead row left unwritten), dead rows are 0, live rows pass the bars and the
    marks are intact (nothing past an output is touched)."""
    import torch
    from twvk_amd import _lib
    from twvk_amd.audio import _ptr, _stream, norm_mode
    hp, basis, wavs, refs = K.row_case(row)
    L = _lib.lib()
    B, n, GUARD, MARK = 3, max(row[4]), 1024, -12345.0
    nbin, n_mels = row[0] // 2 + 1, K.n_mels_of(row)
    x = torch.full((B, n), 7.0, device="cuda:0")                      # past an utterance's length nothing is read
    for b, w in enumerate(wavs):
        x[b, :len(w)] = torch.from_numpy(w).cuda()
    lengths = np.asarray(row[4], np.int32)
    h = C.c_void_p()
    _lib.check(L.twv_spectrogram_create(row[0], row[2], row[1], n_mels, basis.ctypes.data_as(C.c_void_p), n, B, C.byref(h)))
    try:
        T = L.twv_spectrogram_frames(h)
        assert T == _frames(n, hp.hop_size)
        ws = torch.full((L.twv_spectrogram_workspace_bytes(h) // 4 + 64,), float("nan"), device="cuda:0")
        bufs = []
        for width in (n_mels, nbin):
            buf = torch.full((B * T * width + GUARD,), float("nan"), device="cuda:0")
            buf[B * T * width:] = MARK
            bufs.append(buf)
        _lib.check(L.twv_spectrogram_analyze(h, _ptr(x), lengths.ctypes.data_as(C.c_void_p), float(hp.preemphasis), float(hp.ref_level_db),
                                             float(hp.min_level_db), float(hp.max_abs_value), norm_mode(hp), _ptr(ws), _ptr(bufs[0]), _ptr(bufs[1]),
                                             None, _stream()))
        torch.cuda.synchronize()
    finally:
        L.twv_spectrogram_destroy(h)
    outs = []
    for buf, width in zip(bufs, (n_mels, nbin)):
        got = buf.cpu().numpy()
        assert (got[B * T * width:] == MARK).all(), "written behind an output"
        got = got[:B * T * width].reshape(B, T, width)
        assert np.isfinite(got).all(), "an output element was left unwritten"
        outs.append(got)
    mel, lin = outs
    for b, (w, ref) in enumerate(zip(wavs, refs)):
        Tb = _frames(len(w), hp.hop_size)
        _hold(K.measures(mel[b, :Tb], lin[b, :Tb], ref, hp), "%s utterance %d" % (K.row_id(row), b))
        assert not mel[b, Tb:].any() and not lin[b, Tb:].any()
