"""The cases and the bar of the Griffin-Lim tests (tests/test_griffin_lim_cpu.py, tests/test_audio_gpu.py) and of
scripts/griffin_lim_parity.py -- TEST INFRASTRUCTURE ONLY, host code.

Bar of every comparison: e_gpu <= max(8 x e_f32, 1e-6), both e = max|. - float64 checker| / peak(float64 checker) of ONE utterance.
e_f32 is the distance of the checker's own lines run in float32 / complex64 (audio_analysis_ref.inv_spectrogram_f32): what a float32
implementation reaches on THESE inputs.  8 x is the project's margin for another float32 order of operations; the floor, 1e-6 of the
peak, is about 16 float32 spacings at the peak.  Checker runs are cached per case: computed once, shared, never written to."""
import functools

import numpy as np

import audio_analysis_ref as R

MARGIN = 8.0
FLOOR = 1e-6
OLD_BAR = 2e-4            # the bar these tests replaced: no bar may exceed it

# (n_fft, win, hop, T): what it pins
GEOMETRIES = [
    (128, 128, 32, 20),       # no window padding
    (128, 101, 25, 21),       # odd win, odd n_fft - win (pad_center's floor), hop does not divide n_fft
    (64, 32, 40, 12),         # hop > win: samples under a single window, division by one small w^2, samples under none
    (64, 64, 11, 4),          # len 33 = n_fft/2 + 1, the shortest accepted: reflection at its limit on both ends
    (64, 48, 40, 2),          # T = 2
    (2048, 1200, 300, 14),    # the hparams default
]
LONG = (256, 200, 50, 120)                # len 5950: three de-emphasis chunks of 2048
LONG_ITERS = 2
DEEMPH_KS = [0.0, 0.5, 0.97, 0.99, 0.995, 0.999]          # 0.0 = preemphasize off
EDGES = [(128, 128, 32, 65), (128, 128, 32, 66)]          # len 2048 (exactly one chunk) and 2080
EDGE_K = 0.995
BATCH_GEOMETRY = GEOMETRIES[1]
STRIDE = (2048, 1200, 300, 1000)          # x B = 17: 17.4 M bins and 34.8 M frame samples, both past 65 535 blocks of 256
STRIDE_B, STRIDE_DISTINCT = 17, 3


def hparams(n_fft, win, hop, iters, k=0.97, **kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    hp.fft_size, hp.win_size, hp.hop_size, hp.griffin_lim_iters = n_fft, win, hop, iters
    hp.num_freq = n_fft // 2 + 1
    hp.preemphasize, hp.preemphasis = (k != 0.0), (k if k != 0.0 else 0.97)
    for name, v in kw.items():
        setattr(hp, name, v)
    return hp


@functools.lru_cache(maxsize=None)
def inputs(n_fft, T, B, seed, channels=None, lo=-4.5, hi=4.5):
    """(spec (B, T, channels), uniforms (B, T, n_fft/2 + 1)), float32, read-only; beyond +-max_abs_value so that clipping is exercised"""
    rng = np.random.RandomState(seed)
    F = n_fft // 2 + 1
    spec = rng.uniform(lo, hi, (B, T, channels or F)).astype(np.float32)
    u = rng.rand(B, T, F).astype(np.float32)
    spec.setflags(write=False); u.setflags(write=False)
    return spec, u


def seed_of(geometry, iters):
    return 1000 + 7 * GEOMETRIES.index(geometry) + iters if geometry in GEOMETRIES else 2000 + geometry[3] + iters


_cache = {}


def checkers(spec, u, hp, iters, inv_basis=None, key=None):
    """-> (y64, y32) of one utterance, read-only; cached under `key` (hashable) when given"""
    if key is not None and key in _cache:
        return _cache[key]
    y64 = R.inv_spectrogram(spec, u, hp, iters, inv_basis)
    y32 = R.inv_spectrogram_f32(spec, u, hp, iters, inv_basis)
    y64.setflags(write=False); y32.setflags(write=False)
    if key is not None:
        _cache[key] = (y64, y32)
    return y64, y32


def rel(y, y64):
    return float(np.abs(np.asarray(y, np.float64) - y64).max() / np.abs(y64).max())


def bar(e_f32):
    return max(MARGIN * e_f32, FLOOR)


def geometry_case(geometry, iters, B=3, k=0.97):
    """-> (hp, spec, u, [(y64, y32)] per utterance) of one row of the geometry table"""
    n_fft, win, hop, T = geometry
    hp = hparams(n_fft, win, hop, iters, k)
    spec, u = inputs(n_fft, T, B, seed_of(geometry, iters))
    return hp, spec, u, [checkers(spec[b], u[b], hp, iters, key=(geometry, iters, B, k, b)) for b in range(B)]


def long_pre_deemphasis(b=0):
    """the float64 checker's signal BEFORE de-emphasis of utterance b of the long case (5950 samples)"""
    n_fft, win, hop, T = LONG
    spec, u = inputs(n_fft, T, 2, seed_of(LONG, LONG_ITERS))
    return checkers(spec[b], u[b], hparams(n_fft, win, hop, LONG_ITERS, 0.0), LONG_ITERS, key=(LONG, LONG_ITERS, 2, 0.0, b))[0]


def mel_cases():
    """[(name, hp, basis (n_mels, nbin) float32)]: a Slaney basis at n_fft 64, and 300 x 513 random non-negative rows at n_fft 1024
    (both of ga_mel_mag_kernel's loops run more than once; the pseudo-inverse has negative entries, so inv_basis @ amplitudes goes
    below 1e-10 and the clamp works)"""
    hp_a = hparams(64, 64, 16, 0, num_mels=13)
    basis_a = R.mel_basis(hp_a.sample_rate, 64, 13).astype(np.float32)
    hp_b = hparams(1024, 800, 200, 0, num_mels=300)
    basis_b = np.random.RandomState(31).uniform(0.0, 1.0, (300, 513)).astype(np.float32)
    return [("slaney 13x33", hp_a, basis_a), ("random 300x513", hp_b, basis_b)]


def inv_basis_of(basis):
    return np.linalg.pinv(basis.astype(np.float64)).astype(np.float32)
