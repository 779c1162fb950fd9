"""numpy checker of the waveform -> spectrogram path and of the general inverse -- TEST INFRASTRUCTURE ONLY.

Restates utils/audio.py:22-25 (preemphasis), :61-75 (linearspectrogram / melspectrogram), :181-203, :208-234 on top of
oracle.audio_np's librosa.stft restatement (window, centring, framing).  Float64 by default; `dtype=np.float32` runs the SAME lines in
float32 (numpy >= 2 keeps float32 through np.fft.rfft): the measure of what a float32 implementation can reach, which the GPU tests
scale their tolerance by.  The functions pinned to the reference's own code by tests/golden/reference_numpy_audio.npz are
preemphasis, amp_to_db, normalize and denormalize; the mel basis [RECALLED-LIBROSA <= 0.7], written here independently of
twvk_amd.audio.mel_basis, and the STFT conventions are restated from recall.  inv_spectrogram_f32 is the inverse path with every stage,
the Griffin-Lim loop and the de-emphasis included, in float32 / complex64 (scipy.fft): the yardstick of the Griffin-Lim tests."""
import numpy as np

from oracle import audio_np as A


def preemphasis(wav, k):
    """scipy.signal.lfilter([1, -k], [1], wav)"""
    wav = np.asarray(wav)
    out = wav.copy()
    out[1:] = wav[1:] - wav.dtype.type(k) * wav[:-1]
    return out


def amp_to_db(x, min_level_db):
    min_level = np.exp(min_level_db / 20 * np.log(10))
    return 20 * np.log10(np.maximum(x.dtype.type(min_level), x))


def normalize(S, mode, max_abs_value=4.0, min_level_db=-100.0):
    """utils/audio.py:208-220; mode 1 clip + symmetric, 2 clip + asymmetric, 3 symmetric, 4 asymmetric, 0 = signal_normalization off"""
    if mode == 0:
        return S
    if mode == 1:
        return np.clip((2 * max_abs_value) * ((S - min_level_db) / (-min_level_db)) - max_abs_value, -max_abs_value, max_abs_value)
    if mode == 2:
        return np.clip(max_abs_value * ((S - min_level_db) / (-min_level_db)), 0, max_abs_value)
    assert S.max() <= 0 and S.min() - min_level_db >= 0
    if mode == 3:
        return (2 * max_abs_value) * ((S - min_level_db) / (-min_level_db)) - max_abs_value
    return max_abs_value * ((S - min_level_db) / (-min_level_db))


def denormalize(D, mode, max_abs_value=4.0, min_level_db=-100.0):
    """utils/audio.py:222-234, same modes"""
    if mode == 0:
        return D
    if mode == 1:
        return ((np.clip(D, -max_abs_value, max_abs_value) + max_abs_value) * -min_level_db / (2 * max_abs_value)) + min_level_db
    if mode == 2:
        return (np.clip(D, 0, max_abs_value) * -min_level_db / max_abs_value) + min_level_db
    if mode == 3:
        return ((D + max_abs_value) * -min_level_db / (2 * max_abs_value)) + min_level_db
    return (D * -min_level_db / max_abs_value) + min_level_db


def mode_of(hp):
    if not hp.signal_normalization:
        return 0
    if hp.allow_clipping_in_normalization:
        return 1 if hp.symmetric_mels else 2
    return 3 if hp.symmetric_mels else 4


def slaney_hz(mel):
    """mel -> Hz on Slaney's scale: 200/3 Hz per mel up to 1 kHz (15 mel), then a factor 6.4 every 27 mel"""
    return 1000.0 * 6.4 ** ((mel - 15.0) / 27.0) if mel >= 15.0 else mel * 200.0 / 3.0


def slaney_mel(hz):
    return 15.0 + 27.0 * np.log(hz / 1000.0) / np.log(6.4) if hz >= 1000.0 else hz * 3.0 / 200.0


def mel_basis(sr, n_fft, n_mels):
    """librosa.filters.mel(sr, n_fft, n_mels): fmin 0, fmax sr/2, area-normalised triangles -- one filter and one bin at a time"""
    top = slaney_mel(sr / 2.0)
    edges = [slaney_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    out = np.zeros((n_mels, n_fft // 2 + 1))
    for i in range(n_mels):
        lo, mid, hi = edges[i], edges[i + 1], edges[i + 2]
        for k in range(n_fft // 2 + 1):
            f = k * sr / float(n_fft)
            tri = min((f - lo) / (mid - lo), (hi - f) / (hi - mid))
            if tri > 0:
                out[i, k] = tri * 2.0 / (hi - lo)
    return out


def stages(wav, hp, basis=None, dtype=np.float64):
    """every intermediate of utils/audio.py:61-75 for ONE utterance, time-major: x (pre-emphasised), D (frames, bins) complex,
    mag, mel_amp, S_lin, S_mel (dB - ref), lin, mel (normalised; None where the reference's assertion of :216 fires)"""
    dt = np.dtype(dtype).type
    wav = np.asarray(wav, dtype)
    x = preemphasis(wav, hp.preemphasis) if hp.preemphasize else wav
    w = A.hann_padded(hp.win_size, hp.fft_size).astype(dtype)
    xp = np.pad(x, hp.fft_size // 2, mode="reflect")
    n_frames = 1 + (len(xp) - hp.fft_size) // hp.hop_size
    frames = np.stack([xp[i * hp.hop_size:i * hp.hop_size + hp.fft_size] * w for i in range(n_frames)])
    D = np.fft.rfft(frames, axis=1)
    if dtype == np.float64:
        ref = A.stft(x, hp.fft_size, hp.hop_size, hp.win_size)                              # the oracle's own restatement, same lines
        assert np.abs(D.T - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    else:
        assert D.dtype == np.complex64, "numpy < 2 promotes float32 FFTs to float64: the float32 yardstick needs numpy >= 2"
    mag = np.abs(D)
    out = {"x": x, "D": D, "mag": mag}
    mode = mode_of(hp)
    out["S_lin"] = amp_to_db(mag, hp.min_level_db) - dt(hp.ref_level_db)
    if basis is not None:
        out["mel_amp"] = mag @ np.asarray(basis, dtype).T
        out["S_mel"] = amp_to_db(out["mel_amp"], hp.min_level_db) - dt(hp.ref_level_db)
    for name in ("lin", "mel"):
        S = out.get("S_" + name)
        if S is None:
            continue
        try:
            out[name] = normalize(S, mode, dt(hp.max_abs_value), dt(hp.min_level_db))
        except AssertionError:
            out[name] = None
    return out


def spectrograms(wav, hp, basis, dtype=np.float64):
    s = stages(wav, hp, basis, dtype)
    return s["mel"], s["lin"]


def inv_spectrogram(spec, uniforms, hp, iters, inv_basis=None, dtype=np.float64):
    """utils/audio.py:77-110 for ONE utterance, spec (frames, channels), uniforms (frames, bins): _denormalize, _db_to_amp, (for mel:
    max(1e-10, inv_basis @ .)), ** power, then oracle.audio_np's Griffin-Lim and inverse pre-emphasis.  dtype=float32 runs the front
    (up to the fixed magnitudes) in float32 and the loop in float64: the yardstick for the mel front."""
    dt = np.dtype(dtype).type
    D = denormalize(np.asarray(spec, dtype), mode_of(hp), dt(hp.max_abs_value), dt(hp.min_level_db))
    S = np.power(dt(10.0), (D + dt(hp.ref_level_db)) * dt(0.05))
    if inv_basis is not None:
        S = np.maximum(dt(1e-10), S @ np.asarray(inv_basis, dtype).T)
    mag = (S ** dt(hp.power)).astype(np.float64)
    y = A.griffin_lim(mag.T, np.asarray(uniforms, np.float64).T, iters, hp.fft_size, hp.hop_size, hp.win_size)
    return A.inv_preemphasis(y, hp.preemphasis) if hp.preemphasize else y


def inv_preemphasis_f32(wav, k):
    """y[n] = x[n] + k * y[n-1], one sample after the other, every product and sum rounded to float32"""
    wav = np.asarray(wav, np.float32)
    y = np.empty_like(wav)
    k, acc = np.float32(k), np.float32(0.0)
    for i, x in enumerate(wav):
        acc = x + k * acc
        y[i] = acc
    return y


def _stft_f32(y, w, n_fft, hop):
    from scipy import fft as sfft                      # scipy.fft keeps single precision (numpy.fft does not promise to)
    yp = np.pad(y, n_fft // 2, mode="reflect")
    n_frames = 1 + (len(yp) - n_fft) // hop
    frames = np.stack([yp[i * hop:i * hop + n_fft] * w for i in range(n_frames)], axis=1)
    D = sfft.rfft(frames, axis=0)
    assert D.dtype == np.complex64
    return D


def _istft_f32(D, w, hop):
    from scipy import fft as sfft
    n_fft = 2 * (D.shape[0] - 1)
    n_frames = D.shape[1]
    fr = sfft.irfft(D, n_fft, axis=0)
    assert fr.dtype == np.float32
    y = np.zeros(n_fft + hop * (n_frames - 1), np.float32)
    wss = np.zeros_like(y)
    for i in range(n_frames):
        y[i * hop:i * hop + n_fft] += w * fr[:, i]
        wss[i * hop:i * hop + n_fft] += w * w
    nz = wss > np.finfo(np.float32).tiny
    y[nz] /= wss[nz]
    return y[n_fft // 2:len(y) - n_fft // 2]


def inv_spectrogram_f32(spec, uniforms, hp, iters, inv_basis=None):
    """inv_spectrogram with EVERY stage in float32 / complex64 -- denormalise, dB -> amplitude, (inverse basis, max(1e-10, .)),
    ** power, initial phase, istft / stft with a float32 window, unit phase, a sequential float32 de-emphasis: what a float32
    implementation of the same lines reaches, the yardstick of the Griffin-Lim tests.  Restated from oracle/audio_np.py's lines."""
    f = np.float32
    D = denormalize(np.asarray(spec, f), mode_of(hp), f(hp.max_abs_value), f(hp.min_level_db))
    S = np.power(f(10.0), (D + f(hp.ref_level_db)) * f(0.05))
    if inv_basis is not None:
        S = np.maximum(f(1e-10), S @ np.asarray(inv_basis, f).T)
    mag = (S ** f(hp.power)).T
    ph = f(2.0 * np.pi) * np.asarray(uniforms, f).T
    Sc = mag.astype(np.complex64)
    w = A.hann_padded(hp.win_size, hp.fft_size).astype(f)
    y = _istft_f32(Sc * (np.cos(ph) + 1j * np.sin(ph)).astype(np.complex64), w, hp.hop_size)
    for _ in range(iters):
        ang = np.angle(_stft_f32(y, w, hp.fft_size, hp.hop_size))
        y = _istft_f32(Sc * (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64), w, hp.hop_size)
    assert mag.dtype == f and y.dtype == f
    return inv_preemphasis_f32(y, hp.preemphasis) if hp.preemphasize else y


def chunked_deemphasis_model(x, k, chunk=2048, warm=1024):
    """numpy model (float64) of a de-emphasis that restarts the recurrence from a zero state `warm` samples before each `chunk`:
    what ga_deemph_kernel did before it carried the state.  The sensitivity test applies it to show that the Griffin-Lim bars see
    the truncation at k near 1."""
    x = np.asarray(x, np.float64)
    y = np.empty_like(x)
    for n0 in range(0, len(x), chunk):
        acc = 0.0
        for n in range(max(0, n0 - warm), n0):
            acc = x[n] + k * acc
        for n in range(n0, min(n0 + chunk, len(x))):
            acc = x[n] + k * acc
            y[n] = acc
    return y


def parity_signals(sample_rate=24000):
    """the ragged batch of the parity test: lengths 24 000, 23 999 and 7 531 (81, 80 and 26 frames at hop 300) -- a decaying 120 Hz tone
    plus low-passed noise, noise of amplitude 1e-3 (much of its spectrum near min_level), white noise at 0.3"""
    rng = np.random.RandomState(1234)
    t = np.arange(24000) / float(sample_rate)
    tone = 0.5 * np.exp(-3.0 * t) * np.sin(2 * np.pi * 120.0 * t) + 0.05 * np.convolve(rng.randn(24000), np.ones(8) / 8.0, "same")
    return [tone.astype(np.float32), (1e-3 * rng.uniform(-1, 1, 23999)).astype(np.float32), (0.3 * rng.uniform(-1, 1, 7531)).astype(np.float32)]


def noclip_signal(k=0.97):
    """a signal whose every spectrogram value lies inside [min_level_db, 0] dB after the reference level, with room to spare, so that
    the no-clip normalisations accept it (utils/audio.py:216): Gaussian noise through the INVERSE of the pre-emphasis filter, which the
    pre-emphasis turns back into white noise -- every bin's magnitude is then Rayleigh-distributed around 1 (sigma^2 * sum(w^2) = 1.1),
    21 x 1025 values none of which comes near 1e-4 (-100 dB) or 10 (0 dB)."""
    rng = np.random.RandomState(77)
    return A.inv_preemphasis(0.05 * rng.randn(6000), k).astype(np.float32)
