"""Host-side mirror of the reference's audio helpers (utils/audio.py) over the HIP C-ABI, both directions.

    mel, linear = spectrograms(wav, hparams)                      # utils/audio.py:61-75, both from one FFT pass on the GPU
    mel = melspectrogram(wav, hparams); linear = linearspectrogram(wav, hparams)
    wav = inv_linear_spectrogram(linear, hparams, uniforms)      # utils/audio.py:77-92 (synthesizer.py:258), Griffin-Lim on the GPU
    wav = inv_mel_spectrogram(mel, hparams, uniforms)            # utils/audio.py:95-110
    wavs = inv_linear_spectrogram_list([lin_0, lin_1, ...], hparams)   # utterances of unequal lengths in one call (also inv_mel_..._list)
    save_wav(wav, path, hparams.sample_rate)                      # utils/audio.py:14-17 (peak normalisation on the GPU)
    wav = load_wav(path, hparams.sample_rate)                     # utils/audio.py:11-12: any rate, resampled on the GPU
    out, lengths = resample(wavs, 44100, 24000)                   # the resampler behind it, for a ragged batch

Spectrograms are (B, T, channels) throughout: what Tacotron.infer returns and what the npz examples hold (the reference works on one
utterance at a time, transposed to (channels, T)).  PyTorch is used for device memory and streams only."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .wavenet import _ptr, _stream


def norm_mode(hparams):
    """the C-ABI's norm_mode for _normalize / _denormalize (utils/audio.py:208-234)"""
    if not hparams.signal_normalization:
        return 0
    if hparams.allow_clipping_in_normalization:
        return 1 if hparams.symmetric_mels else 2
    return 3 if hparams.symmetric_mels else 4


def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(m >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (m - min_log_hz / f_sp)), f_sp * m)


def mel_basis(hparams):
    """utils/audio.py:193-199 `librosa.filters.mel(sample_rate, fft_size, n_mels=num_mels)` -> float32 (num_mels, fft_size/2 + 1).
    [RECALLED-LIBROSA <= 0.7]: fmin = 0, fmax = sr/2, Slaney's scale (200/3 Hz per mel below 1 kHz, log step ln(6.4)/27 above),
    num_mels + 2 band edges equally spaced in mel, triangles min(rising, falling) clipped at 0 and scaled by 2 / (f[i+2] - f[i]).
    Computed in float64 on the host; the kernels take any basis (twv_spectrogram_create), so librosa's own matrix can be passed."""
    sr, n_fft, n_mels = float(hparams.sample_rate), int(hparams.fft_size), int(hparams.num_mels)
    fft_f = np.linspace(0.0, sr / 2, 1 + n_fft // 2)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sr / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return weights.astype(np.float32)


_basis_cache = {}
_analyzers = {}          # (device, n_fft, hop, win, basis key, max_samples, batch) -> [handle, workspace]: the FFT plan lives in the handle
_MAX_ANALYZERS = 4


def _default_basis(hparams):
    key = (hparams.sample_rate, hparams.fft_size, hparams.num_mels)
    if key not in _basis_cache:
        _basis_cache[key] = mel_basis(hparams)
    return key, _basis_cache[key]


def _analyzer(L, hparams, basis_key, basis, max_samples, batch, device):
    key = (str(device), hparams.fft_size, hparams.hop_size, hparams.win_size, basis_key, max_samples, batch)
    hit = _analyzers.pop(key, None)
    if hit is None:
        h = C.c_void_p()
        _lib.check(L.twv_spectrogram_create(hparams.fft_size, hparams.hop_size, hparams.win_size, basis.shape[0],
                                            basis.ctypes.data_as(C.c_void_p), max_samples, batch, C.byref(h)))
        hit = [h, torch.empty(L.twv_spectrogram_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device=device)]
        while len(_analyzers) >= _MAX_ANALYZERS:                 # oldest first (dicts keep insertion order)
            old = _analyzers.pop(next(iter(_analyzers)))
            torch.cuda.synchronize(device)
            L.twv_spectrogram_destroy(old[0])
    _analyzers[key] = hit
    return hit


def _as_batch(wav, lengths, device):
    """(len,), (B, len), a list of 1-D arrays, or a device tensor -> ((B, max_len) float32 device tensor, int32 lengths, was 1-D)"""
    if isinstance(wav, (list, tuple)) and len(wav) and np.ndim(wav[0]) == 1:
        if lengths is not None:
            raise ValueError("a list of utterances carries its own lengths")
        lengths = np.asarray([len(w) for w in wav], np.int32)
        host = np.zeros((len(wav), int(lengths.max())), np.float32)
        for b, w in enumerate(wav):
            host[b, :len(w)] = np.asarray(w, np.float32)
        return torch.from_numpy(host).to(device), lengths, False
    x = torch.as_tensor(wav, dtype=torch.float32, device=device)
    single = x.dim() == 1
    if single:
        x = x[None]
    if x.dim() != 2:
        raise ValueError("wav must be (len,), (B, len) or a list of 1-D arrays")
    x = x.contiguous()
    if lengths is None:
        lengths = np.full(x.shape[0], x.shape[1], np.int32)
    lengths = np.ascontiguousarray(lengths, np.int32).reshape(-1)
    if len(lengths) != x.shape[0]:
        raise ValueError("lengths must have one entry per utterance")
    return x, lengths, single


def spectrograms(wav, hparams, lengths=None, mel_basis=None, device="cuda:0", mel=True, linear=True):
    """utils/audio.py:61-75 for a ragged batch, both outputs from one FFT pass (twv_spectrogram_analyze):
    -> (mel (B, frames, num_mels), linear (B, frames, fft_size/2 + 1)), frames = 1 + max(len) // hop_size; an utterance of `len`
    samples fills its first 1 + len // hop_size rows, the rest are 0.  The reference returns (channels, frames) for one utterance.
    wav: (len,) (then the outputs have no batch axis), (B, len) with optional `lengths`, or a list of 1-D arrays of different lengths;
    a tensor already on the device is used in place.  mel_basis: (num_mels, fft_size/2 + 1), default mel_basis(hparams).
    The no-clip normalisations raise AssertionError where utils/audio.py:216 does."""
    if getattr(hparams, "use_lws", False):
        raise NotImplementedError("use_lws=True (hparams.py:15 default False) is not built")
    if not (mel or linear):
        raise ValueError("neither output requested")
    if isinstance(wav, torch.Tensor) and wav.is_cuda:
        device = wav.device
    x, lengths, single = _as_batch(wav, lengths, device)
    B, n = x.shape
    if mel_basis is None:
        bkey, basis = _default_basis(hparams)
    else:
        basis = np.ascontiguousarray(mel_basis, np.float32)
        if basis.shape != (hparams.num_mels, hparams.fft_size // 2 + 1):
            raise ValueError("mel_basis must be (num_mels, fft_size/2 + 1) = %s" % ((hparams.num_mels, hparams.fft_size // 2 + 1),))
        import hashlib
        bkey = hashlib.sha1(basis.tobytes()).hexdigest()
    mode = norm_mode(hparams)
    L = _lib.lib()
    with torch.cuda.device(x.device):
        h, ws = _analyzer(L, hparams, bkey, basis, n, B, x.device)
        T = L.twv_spectrogram_frames(h)
        mel_out = torch.empty((B, T, basis.shape[0]), dtype=torch.float32, device=x.device) if mel else None
        lin_out = torch.empty((B, T, hparams.fft_size // 2 + 1), dtype=torch.float32, device=x.device) if linear else None
        mm = torch.empty(2, dtype=torch.float32, device=x.device) if mode in (3, 4) else None
        _lib.check(L.twv_spectrogram_analyze(h, _ptr(x), lengths.ctypes.data_as(C.c_void_p),
                                             float(hparams.preemphasis) if hparams.preemphasize else 0.0, float(hparams.ref_level_db),
                                             float(hparams.min_level_db), float(hparams.max_abs_value), mode, _ptr(ws),
                                             _ptr(mel_out) if mel else None, _ptr(lin_out) if linear else None,
                                             _ptr(mm) if mm is not None else None, _stream()))
        if mm is not None:
            lo, hi = mm.tolist()
            assert hi <= 0 and lo - hparams.min_level_db >= 0, \
                "utils/audio.py:216: S.max() = %g, S.min() = %g outside [min_level_db, 0] without clipping" % (hi, lo)
    if single:
        mel_out = mel_out[0] if mel else None
        lin_out = lin_out[0] if linear else None
    return mel_out, lin_out


def melspectrogram(wav, hparams, lengths=None, mel_basis=None, device="cuda:0"):
    """utils/audio.py:69-75 -> (B, frames, num_mels); see spectrograms"""
    return spectrograms(wav, hparams, lengths, mel_basis, device, linear=False)[0]


def linearspectrogram(wav, hparams, lengths=None, device="cuda:0"):
    """utils/audio.py:61-67 -> (B, frames, fft_size/2 + 1); see spectrograms"""
    return spectrograms(wav, hparams, lengths, None, device, mel=False)[1]


_resamplers = {}         # (device, orig_sr, target_sr, max_samples_in, batch) -> [handle, workspace]: the table lives in the workspace
_MAX_RESAMPLERS = 4


def _resampler(L, orig_sr, target_sr, max_in, batch, device):
    key = (str(device), orig_sr, target_sr, max_in, batch)
    hit = _resamplers.pop(key, None)
    if hit is None:
        h = C.c_void_p()
        _lib.check(L.twv_resample_create(orig_sr, target_sr, max_in, batch, C.byref(h)))
        hit = [h, torch.empty(L.twv_resample_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device=device)]
        while len(_resamplers) >= _MAX_RESAMPLERS:               # oldest first
            old = _resamplers.pop(next(iter(_resamplers)))
            torch.cuda.synchronize(device)
            L.twv_resample_destroy(old[0])
    _resamplers[key] = hit
    return hit


def _as_frames(wav, lengths, device):
    """-> ((B, max_len[, 2]) int16 or float32 device tensor, int32 lengths).  A list holds utterances, (len,) or (len, 2) each;
    an array or tensor is (len,), (B, len) or (B, len, 2) -- one stereo utterance is passed as [x] or x[None]."""
    if isinstance(wav, (list, tuple)):
        if lengths is not None:
            raise ValueError("a list of utterances carries its own lengths")
        if not len(wav):
            raise ValueError("no utterances")
        arrs = [w.cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w) for w in wav]
        tail = arrs[0].shape[1:]
        if any(a.ndim not in (1, 2) or a.shape[1:] != tail for a in arrs) or tail not in ((), (2,)):
            raise ValueError("utterances must all be (len,) or all be (len, 2)")
        dt = np.int16 if all(a.dtype == np.int16 for a in arrs) else np.float32
        if dt is np.float32 and any(a.dtype.kind != "f" for a in arrs):
            raise ValueError("utterances must all be int16 or all be floating point")
        lengths = np.asarray([len(a) for a in arrs], np.int32)
        host = np.zeros((len(arrs), max(1, int(lengths.max()))) + tail, dt)
        for b, a in enumerate(arrs):
            host[b, :len(a)] = a
        return torch.from_numpy(host).to(device), lengths
    x = wav if isinstance(wav, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(wav))
    if x.dtype != torch.int16:
        if not x.dtype.is_floating_point:
            raise ValueError("samples must be int16 or floating point, got %s" % (x.dtype,))
        x = x.to(torch.float32)
    x = x.to(device)
    if x.dim() == 1:
        x = x[None]
    if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[2] != 2) or x.shape[1] < 1:
        raise ValueError("wav must be (len,), (B, len), (B, len, 2) or a list of utterances")
    x = x.contiguous()
    if lengths is None:
        lengths = np.full(x.shape[0], x.shape[1], np.int32)
    lengths = np.ascontiguousarray(lengths, np.int32).reshape(-1)
    if len(lengths) != x.shape[0]:
        raise ValueError("lengths must have one entry per utterance")
    return x, lengths


def resample(wav, orig_sr, target_sr, lengths=None, device="cuda:0"):
    """What librosa.core.load does after reading (utils/audio.py:11-12): channels averaged, then band-limited resampling
    orig_sr -> target_sr, for a ragged batch in one kernel (twv_resample; the arithmetic is DESIGN.md's "Resampling" contract,
    [RECALLED] resampy's kaiser_best parameters, unpinned against librosa).
    wav: what `spectrograms` accepts -- (len,), (B, len) with optional `lengths`, a list of 1-D arrays, a device tensor -- and also
    int16 samples (scaled by 1 / 32768 on the device) and interleaved stereo as (B, len, 2) or a list of (len, 2) arrays.
    -> ((B, max_out) float32 device tensor, zero past each utterance's end, [out length per utterance]),
    out length = ceil(len * target_sr / orig_sr).  Equal rates: (wav, lengths) come back as given, nothing is launched."""
    orig_sr, target_sr = int(orig_sr), int(target_sr)
    if orig_sr == target_sr:
        return wav, lengths
    if isinstance(wav, torch.Tensor) and wav.is_cuda:
        device = wav.device
    x, lengths = _as_frames(wav, lengths, device)
    B, n = x.shape[0], x.shape[1]
    L = _lib.lib()
    with torch.cuda.device(x.device):
        h, ws = _resampler(L, orig_sr, target_sr, n, B, x.device)
        out = torch.empty((B, L.twv_resample_out_samples(h, n)), dtype=torch.float32, device=x.device)
        _lib.check(L.twv_resample(h, _ptr(x), 1 if x.dtype == torch.int16 else 0, 2 if x.dim() == 3 else 1,
                                  lengths.ctypes.data_as(C.c_void_p), _ptr(ws), _ptr(out), _stream()))
        out_lengths = [int(L.twv_resample_out_samples(h, int(v))) for v in lengths]
    return out, out_lengths


def wav_samples(data):
    """what scipy.io.wavfile.read returns -> what `resample` takes: int16 as it is (the device scales it by 1 / 32768), every other
    format as float32 in [-1, 1); one or two channels are kept, more are averaged here"""
    if data.dtype == np.int32:
        data = (data.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif data.dtype == np.float64:
        data = data.astype(np.float32)
    elif data.dtype == np.uint8:
        data = (data.astype(np.float32) - 128.0) / 128.0
    elif data.dtype not in (np.int16, np.float32):
        raise ValueError("unsupported sample format %s (uint8, int16, int32 and float wavs are read)" % (data.dtype,))
    if data.ndim == 2 and data.shape[1] == 1:
        data = data[:, 0]
    if data.ndim == 2 and data.shape[1] > 2:
        data = (data.astype(np.float32) / 32768.0 if data.dtype == np.int16 else data).mean(axis=1)
    return data


def load_wav(path, sr, device="cuda:0"):
    """utils/audio.py:11-12 `librosa.core.load(path, sr=sr)[0]`: float32 numpy at `sr`, channels averaged; a file of another rate
    is resampled on the GPU (`resample`)."""
    from scipy.io import wavfile
    rate, data = wavfile.read(path)
    x = wav_samples(data)
    if rate == sr:
        x = x.astype(np.float32) / 32768.0 if x.dtype == np.int16 else x
        return x.mean(axis=1) if x.ndim == 2 else x
    out, n = resample([x], rate, sr, device=device)
    return out[0, :n[0]].cpu().numpy()


def _griffin_lim(spec, inv_basis, hparams, uniforms, seed, general):
    B, T, _ = spec.shape
    F = hparams.fft_size // 2 + 1
    if uniforms is None:
        uniforms = np.random.RandomState(seed).rand(B, T, F)
    u = torch.as_tensor(uniforms, dtype=torch.float32, device=spec.device).contiguous()
    if tuple(u.shape) != (B, T, F):
        raise ValueError("uniforms must be %s" % ((B, T, F),))
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_griffin_lim_create(hparams.fft_size, hparams.hop_size, hparams.win_size, T, B, C.byref(h)))
    try:
        with torch.cuda.device(spec.device):
            n = L.twv_griffin_lim_samples(h)
            ws = torch.empty(L.twv_griffin_lim_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device=spec.device)
            out = torch.empty((B, n), dtype=torch.float32, device=spec.device)
            k = float(hparams.preemphasis) if hparams.preemphasize else 0.0
            if general:
                _lib.check(L.twv_inv_spectrogram(h, _ptr(spec), spec.shape[2], _ptr(inv_basis) if inv_basis is not None else None, _ptr(u),
                                                 int(hparams.griffin_lim_iters), float(hparams.power), float(hparams.ref_level_db),
                                                 float(hparams.max_abs_value), float(hparams.min_level_db), norm_mode(hparams), k,
                                                 _ptr(ws), _ptr(out), _stream()))
            else:
                _lib.check(L.twv_inv_linear_spectrogram(h, _ptr(spec), _ptr(u), int(hparams.griffin_lim_iters), float(hparams.power),
                                                        float(hparams.ref_level_db), float(hparams.max_abs_value), float(hparams.min_level_db),
                                                        k, _ptr(ws), _ptr(out), _stream()))
            torch.cuda.current_stream().synchronize()
    finally:
        L.twv_griffin_lim_destroy(h)
    return out


def inv_linear_spectrogram(linear, hparams, uniforms=None, seed=None, device="cuda:0"):
    """(B, T, num_freq) normalised linear spectrograms -> (B, hop_size*(T-1)) waveforms.
    uniforms (B, T, num_freq) in [0,1) replace utils/audio.py:131 np.random.rand; drawn from `seed` when absent.
    Every normalisation setting of _denormalize (utils/audio.py:222-234); the default one takes twv_inv_linear_spectrogram."""
    if getattr(hparams, "use_lws", False):
        raise NotImplementedError("use_lws=True (hparams.py:15 default False) is not built")
    lin = torch.as_tensor(linear, dtype=torch.float32, device=device).contiguous()
    if lin.dim() == 2:
        lin = lin[None]
    B, T, F = lin.shape
    if F != hparams.fft_size // 2 + 1:
        raise ValueError("last dimension must be fft_size/2 + 1 = %d, got %d" % (hparams.fft_size // 2 + 1, F))
    return _griffin_lim(lin, None, hparams, uniforms, seed, general=norm_mode(hparams) != 1)


def inv_mel_spectrogram(mel, hparams, uniforms=None, seed=None, mel_basis=None, device="cuda:0"):
    """utils/audio.py:95-110: (B, T, num_mels) normalised mel spectrograms -> (B, hop_size*(T-1)) waveforms through
    _mel_to_linear (:187-191, inv_basis = np.linalg.pinv(mel basis), float64 on the host) and the same Griffin-Lim loop.
    uniforms (B, T, fft_size/2 + 1) as in inv_linear_spectrogram."""
    if getattr(hparams, "use_lws", False):
        raise NotImplementedError("use_lws=True (hparams.py:15 default False) is not built")
    m = torch.as_tensor(mel, dtype=torch.float32, device=device).contiguous()
    if m.dim() == 2:
        m = m[None]
    basis = _default_basis(hparams)[1] if mel_basis is None else np.asarray(mel_basis)
    if m.shape[2] != basis.shape[0] or basis.shape[1] != hparams.fft_size // 2 + 1:
        raise ValueError("mel is (B, T, %d) but the basis is %s" % (m.shape[2], basis.shape))
    inv = torch.as_tensor(np.linalg.pinv(basis.astype(np.float64)).astype(np.float32), device=m.device).contiguous()
    return _griffin_lim(m, inv, hparams, uniforms, seed, general=True)


def _shape(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _packed(arrays, device):
    """a list of (T_i, C) arrays or tensors -> one contiguous (sum T_i, C) float32 device tensor"""
    if not any(isinstance(a, torch.Tensor) for a in arrays):
        return torch.from_numpy(np.concatenate([np.asarray(a, np.float32) for a in arrays], axis=0)).to(device)
    return torch.cat([torch.as_tensor(a, dtype=torch.float32, device=device) for a in arrays], dim=0).contiguous()


def _griffin_lim_list(specs, channels, basis, hparams, uniforms, seed, general, device):
    """the list fronts below: every argument is checked on the host first (ValueError, no device work), then ONE ragged handle
    (twv_griffin_lim_create_ragged) runs all utterances packed end to end -> 1-D views of one (total_samples,) tensor"""
    if getattr(hparams, "use_lws", False):
        raise ValueError("use_lws=True (hparams.py:15 default False) is not built")
    if not isinstance(specs, (list, tuple)) or not len(specs):
        raise ValueError("a non-empty list of (T_i, %d) spectrograms is required" % channels)
    F = hparams.fft_size // 2 + 1
    Ts = []
    for i, s in enumerate(specs):
        shp = _shape(s)
        if len(shp) != 2 or shp[1] != channels:
            raise ValueError("utterance %d must be (T, %d), got %s" % (i, channels, shp))
        if shp[0] < 2 or hparams.hop_size * (shp[0] - 1) <= hparams.fft_size // 2:
            raise ValueError("utterance %d: %d frames are %d samples, not more than the reflect padding (fft_size/2 = %d)"
                             % (i, shp[0], hparams.hop_size * max(shp[0] - 1, 0), hparams.fft_size // 2))
        Ts.append(int(shp[0]))
    if uniforms is None:
        rs = np.random.RandomState(seed)
        uniforms = [rs.rand(T, F) for T in Ts]                   # a list of one: the stream of rand(1, T, F)
    elif not isinstance(uniforms, (list, tuple)) or [_shape(u) for u in uniforms] != [(T, F) for T in Ts]:
        raise ValueError("uniforms must be a list of %s" % ([(T, F) for T in Ts],))
    device = torch.device(device)
    for t in list(specs) + list(uniforms):
        if isinstance(t, torch.Tensor) and t.is_cuda:
            device = t.device
            break
    L = _lib.lib()
    h = C.c_void_p()
    n_frames = np.asarray(Ts, np.int32)
    _lib.check(L.twv_griffin_lim_create_ragged(hparams.fft_size, hparams.hop_size, hparams.win_size, n_frames.ctypes.data_as(C.c_void_p),
                                               len(Ts), C.byref(h)))
    try:
        with torch.cuda.device(device):
            spec = _packed(specs, device)
            u = _packed(uniforms, device)
            inv_basis = None
            if basis is not None:                                # utils/audio.py:187-191 _mel_to_linear, as inv_mel_spectrogram does
                inv_basis = torch.as_tensor(np.linalg.pinv(basis.astype(np.float64)).astype(np.float32), device=device).contiguous()
            s_off = (C.c_int64 * (len(Ts) + 1))()
            _lib.check(L.twv_griffin_lim_offsets(h, None, C.cast(s_off, C.c_void_p)))
            ws = torch.empty(L.twv_griffin_lim_workspace_bytes(h) // 4 + 64, dtype=torch.float32, device=device)
            out = torch.empty(L.twv_griffin_lim_total_samples(h), dtype=torch.float32, device=device)
            k = float(hparams.preemphasis) if hparams.preemphasize else 0.0
            if general:
                _lib.check(L.twv_inv_spectrogram(h, _ptr(spec), channels, _ptr(inv_basis) if inv_basis is not None else None, _ptr(u),
                                                 int(hparams.griffin_lim_iters), float(hparams.power), float(hparams.ref_level_db),
                                                 float(hparams.max_abs_value), float(hparams.min_level_db), norm_mode(hparams), k,
                                                 _ptr(ws), _ptr(out), _stream()))
            else:
                _lib.check(L.twv_inv_linear_spectrogram(h, _ptr(spec), _ptr(u), int(hparams.griffin_lim_iters), float(hparams.power),
                                                        float(hparams.ref_level_db), float(hparams.max_abs_value), float(hparams.min_level_db),
                                                        k, _ptr(ws), _ptr(out), _stream()))
            torch.cuda.current_stream().synchronize()
    finally:
        L.twv_griffin_lim_destroy(h)
    return [out[s_off[b]:s_off[b + 1]] for b in range(len(Ts))]


def inv_linear_spectrogram_list(linears, hparams, uniforms=None, seed=None, device="cuda:0"):
    """inv_linear_spectrogram for utterances of unequal lengths in ONE call: linears is a list of (T_i, num_freq) arrays or tensors
    -> a list of 1-D tensors of hop_size * (T_i - 1) samples, views of one packed buffer.  Every utterance comes out as from a call
    of its own (overlap-add, reflect padding and the de-emphasis state stop at its ends); the number of kernel launches does not
    depend on the list.  uniforms: a list of (T_i, num_freq); without it `rs = RandomState(seed); [rs.rand(T_i, num_freq) ...]`.
    ValueError before any device work: an empty list, a wrong channel count, uniforms of other shapes, an utterance not longer
    than the reflect padding (hop_size * (T_i - 1) <= fft_size / 2), use_lws."""
    return _griffin_lim_list(linears, hparams.fft_size // 2 + 1, None, hparams, uniforms, seed, norm_mode(hparams) != 1, device)


def inv_mel_spectrogram_list(mels, hparams, uniforms=None, seed=None, mel_basis=None, device="cuda:0"):
    """inv_mel_spectrogram for a list of (T_i, num_mels) mel spectrograms; see inv_linear_spectrogram_list (uniforms are
    (T_i, fft_size/2 + 1) here too)"""
    basis = _default_basis(hparams)[1] if mel_basis is None else np.asarray(mel_basis)
    if basis.ndim != 2 or basis.shape[1] != hparams.fft_size // 2 + 1:
        raise ValueError("the basis is %s, not (num_mels, %d)" % (basis.shape, hparams.fft_size // 2 + 1))
    return _griffin_lim_list(mels, basis.shape[0], basis, hparams, uniforms, seed, True, device)


def save_wav(wav, path, sr):
    """utils/audio.py:14-17"""
    from scipy.io import wavfile
    from .ops import wav_to_int16
    wavfile.write(path, sr, wav_to_int16(wav).cpu().numpy().reshape(-1))
