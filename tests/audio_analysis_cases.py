"""The geometry table, the signals and the two measures of the waveform -> spectrogram tests (tests/test_audio_analysis_cpu.py,
tests/test_audio_analysis_geometry_gpu.py) and of scripts/audio_analysis_parity.py -- TEST INFRASTRUCTURE ONLY, host code.

Two measures per utterance and output (mel, linear); both must hold.
  dB bar         max|gpu - f64| <= max(8 x max|f32 checker - f64|, 1e-5) in normalised units: test_audio_analysis_gpu._bar's, unchanged.
                 Near min_level a float32 FFT's absolute error is a large relative one, so this bar is loose (up to 1e-2 at n_fft 8190)
                 exactly where a wrong strong bin could hide.
  amplitude bar  a(x) = 10 ** ((denormalize(x) + ref_level_db) / 20) in float64, e = max|a(.) - a(f64)| / max a(f64);
                 e_gpu <= max(8 x e_f32, 1e-6) (griffin_lim_cases.MARGIN and FLOOR).  The float32 FFT's error is absolute -- about eps x
                 the frame's norm -- so this measure is uniform over the bins and a strong bin cannot hide.
e_f32 is the distance of the checker's own lines run in float32: what a float32 implementation reaches on THESE inputs.  Checker runs
are cached per (row, utterance): computed once, shared, never written to."""
import functools

import numpy as np

import audio_analysis_ref as R
from griffin_lim_cases import FLOOR, MARGIN

AMP_BAR_CAP = 2e-5        # no amplitude bar may exceed it (tests/test_audio_analysis_cpu.py): e_f32 <= 2.5e-6
SAMPLE_RATE = 24000
DENSE = "dense 300x513"

# (n_fft, win, hop, basis, the lengths of a ragged batch of three): what it pins in csrc/twv_audio_analysis.hip.  basis = the number of
# Slaney filters, or DENSE
TABLE = [
    (128, 128, 32, 20, (700, 66, 65)),            # lpad 0; nbin 65 < 256: most threads of sa_output_kernel have no bin; the shortest accepted signal (65)
    (128, 101, 25, 13, (500, 410, 65)),           # odd win, odd n_fft - win, hop does not divide n_fft
    (64, 32, 40, 8, (400, 33, 399)),              # hop > win
    (64, 64, 11, 8, (33, 34, 120)),               # len 33 = n_fft/2 + 1: sa_sample's single reflection at its limit on both ends
    (64, 48, 100, 8, (99, 40, 33)),               # hop > len: one frame per utterance, frames = 1
    (64, 64, 16, 40, (300, 33, 100)),             # 10 of the 40 filters are empty (count == 0)
    (126, 100, 30, 12, (600, 64, 333)),           # sa_frame_kernel<2> (n_fft % 4 == 2), FFT length 2 * 3^2 * 7
    (2058, 1200, 300, 80, (4000, 1030, 2999)),    # <2> at size; nbin 1030: a second trip of the `base` loop with six threads; 2 * 3 * 7^3
    (8190, 8190, 2048, 80, (9000, 4096, 8191)),   # the largest accepted n_fft: 65 536 bytes of sa_mag, 32 760 of sa_prod; 2 * 3^2 * 5 * 7 * 13
    (1024, 800, 200, DENSE, (3000, 513, 1999)),   # n_mels > 256; dense rows; an all-zero row; a narrow band
]
ALONE_ROWS = [TABLE[1], TABLE[3], TABLE[6], TABLE[9]]
ONE_OUTPUT_ROWS = [TABLE[6], TABLE[5]]
SETTINGS_ROW = TABLE[6]
STALE_ROWS = [TABLE[4], TABLE[6], TABLE[7]]


def row_id(row):
    return "%d-%d-%d-%s" % (row[0], row[1], row[2], "dense" if row[3] == DENSE else "slaney%d" % row[3])


def n_mels_of(row):
    return 300 if row[3] == DENSE else row[3]


def hparams(row, **kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    hp.fft_size, hp.win_size, hp.hop_size = row[0], row[1], row[2]
    hp.num_freq, hp.num_mels = row[0] // 2 + 1, n_mels_of(row)
    hp.sample_rate, hp.preemphasize, hp.preemphasis = SAMPLE_RATE, True, 0.97
    for name, v in kw.items():
        setattr(hp, name, v)
    return hp


@functools.lru_cache(maxsize=None)
def basis(row):
    """(n_mels, n_fft/2 + 1) float32, read-only: the SAME matrix goes to the device (mel_basis=) and to the checker, so the basis itself
    is not what is compared"""
    n_fft = row[0]
    if row[3] == DENSE:
        b = (np.random.RandomState(31).uniform(0.0, 1.0, (300, n_fft // 2 + 1)) * 1e-3).astype(np.float32)
        b[7] = 0.0                                # count == 0 in a dense basis
        b[100, :200] = 0.0; b[100, 260:] = 0.0    # a narrow band: first = 200, count = 60
    else:
        b = R.mel_basis(SAMPLE_RATE, n_fft, row[3]).astype(np.float32)
    b.setflags(write=False)
    return b


def empty_filters(row):
    return int((~basis(row).any(axis=1)).sum())


# One seed per utterance, found on the float64 checker ALONE: the first of 1000 * row + 100 * utterance + 0, 1, 2, ... for which no
# checker value sits on a clip edge (the conditions tests/test_audio_analysis_cpu.py asserts).  Seeds have to be chosen: frame 0 of
# every utterance is an even sequence (the reflect padding mirrors about sample 0), so its spectrum is real, and a real Gaussian bin
# falls below min_level about once in 10^4 -- at 4096 bins, in most utterances.
SEEDS = [(0, 100, 200), (1000, 1100, 1200), (2000, 2100, 2200), (3000, 3100, 3200), (4000, 4100, 4200), (5001, 5100, 5200),
         (6000, 6100, 6200), (7000, 7102, 7200), (8001, 8108, 8202), (9003, 9100, 9200)]


@functools.lru_cache(maxsize=None)
def signals(row):
    """the ragged batch of a row: g (0.3 sin(2 pi 0.013 t) sin^2(pi t / n) + 0.02 randn) per utterance, float32, read-only.
    g = min(1, 1600 / win): the tone's bin holds about 0.3 * win / 4 * 0.086 (the pre-emphasis filter's gain at 0.013 cycles per
    sample), which passes 10 = 0 dB after the reference level -- the upper clip edge -- at win 1550; g keeps it below at win 8190."""
    out = []
    g = min(1.0, 1600.0 / row[1])
    for n, seed in zip(row[4], SEEDS[TABLE.index(row)]):
        t = np.arange(n)
        x = 0.3 * np.sin(2 * np.pi * 0.013 * t) * np.sin(np.pi * t / n) ** 2 + 0.02 * np.random.RandomState(seed).randn(n)
        x = (g * x).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


_cache = {}


def checkers(wav, hp, mel_basis, key=None):
    """-> (mel64, lin64, mel32, lin32) of one utterance, read-only (None where the reference's assertion fires); cached under `key`.
    The float64 run carries the checker's own assertion against oracle.audio_np.stft (audio_analysis_ref.stages)."""
    if key is not None and key in _cache:
        return _cache[key]
    out = R.spectrograms(wav, hp, mel_basis) + R.spectrograms(wav, hp, mel_basis, dtype=np.float32)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    if key is not None:
        _cache[key] = out
    return out


def row_case(row):
    """-> (hp, basis, wavs, [(mel64, lin64, mel32, lin32)] per utterance) of one row, default normalisation"""
    hp, b, wavs = hparams(row), basis(row), signals(row)
    return hp, b, wavs, [checkers(w, hp, b, key=(row, i)) for i, w in enumerate(wavs)]


def amplitude(x, hp):
    """a normalised (or, signal_normalization off, dB) spectrogram back to amplitudes, float64"""
    S = R.denormalize(np.asarray(x, np.float64), R.mode_of(hp), float(hp.max_abs_value), float(hp.min_level_db))
    return 10.0 ** ((S + float(hp.ref_level_db)) / 20.0)


def amp_rel(x, x64, hp):
    """e of the amplitude measure"""
    a64 = amplitude(x64, hp)
    return float(np.abs(amplitude(x, hp) - a64).max() / a64.max())


def amp_bar(e_f32):
    return max(MARGIN * e_f32, FLOOR)


def db_bar(x32, x64, floor=1e-5):
    """test_audio_analysis_gpu._bar's expression for one output -> (bar, the float32 checker's distance)"""
    d = float(np.abs(x32 - x64).max())
    return max(8 * d, floor), d


def measures(got_mel, got_lin, ref, hp, floor=1e-5):
    """one utterance: [(output name, dB distance, f32 checker's, dB bar, e, e_f32, amplitude bar)] for mel and linear; an output passed
    as None is left out"""
    m64, l64, m32, l32 = ref
    out = []
    for name, got, x64, x32 in (("mel", got_mel, m64, m32), ("linear", got_lin, l64, l32)):
        if got is None:
            continue
        got = np.asarray(got)
        assert got.shape == x64.shape, (name, got.shape, x64.shape)
        bar, d32 = db_bar(x32, x64, floor)
        e32 = amp_rel(x32, x64, hp)
        out.append((name, float(np.abs(got - x64).max()), d32, bar, amp_rel(got, x64, hp), e32, amp_bar(e32)))
    return out
