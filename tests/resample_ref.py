"""float64 numpy checker of the resampling contract ("Resampling"; include/twv_amd.h): direct evaluation, np.sinc and
np.i0 per tap, no table look-up and no scipy.

    g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, s = min(1, L / M);  n_out = ceil(n_in * L / M)
    y[t] = sum_n x[n] * s * h(s * (t * M / L - n)),  x zero outside [0, n_in),  t * M = q * L + p in integers
    h(u) = r sinc(r u) I0(beta sqrt(1 - (u / Z)^2)) / I0(beta) for |u| < Z, else 0        [RECALLED: resampy's kaiser_best]

dtype=np.float32 rounds the coefficients once and forms and sums the products in float32 (numpy's pairwise sum, the tighter of the
orders tried: 1.4-2.3e-7 of the peak on 30 000 samples of noise, where one running sum gives 0.5-1.1e-6): the measure the tests' bar
is taken from."""
from math import gcd

import numpy as np

ZEROS, ROLLOFF, BETA = 64, 0.9475937167399596, 14.769656459379492
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000)
PAIRS = ((44100, 24000), (48000, 24000), (16000, 24000), (22050, 24000), (8000, 24000), (24000, 16000), (44100, 16000),
         # one pair for every route of the kernel the seven above leave out (ROUTES below)
         (11025, 32000), (32000, 11025), (96000, 11025), (96000, 44100), (16000, 11025), (96000, 8000))
RATIO, FLOOR = 8.0, 5e-6            # tests/train_cases.py: float32 sums in another order

# What twv_resample_create decides per pair, held as the expected table (tests/test_resample_cpu.py asserts it on the host):
# pair -> (L, M, taps, LR, chunks, lanes of a wave that are not live, LDS bytes of a workgroup).  LR is the instantiation
# rs_resample_kernel<LR>; rounds per workgroup = LR * chunks; a wave holds 64 / LR phases, so L % (64 / LR) phases of the last wave's
# are live and the rest of its lanes are not.  What each of the added pairs pins:
#   11025 -> 32000  <4>, upsampling                    32000 -> 11025  <4>, chunks 2, lanes that are not live
#   96000 -> 11025  <4>, 1120 taps, a wave almost all dead            96000 -> 44100  <16>, chunks 2, lanes that are not live
#   16000 -> 11025  <16> with more than 64 KiB of LDS                 96000 -> 8000   <64>, 1536 taps, L = 1
ROUTES = {
    (44100, 24000): (80, 147, 240, 64, 1, 0, 59716),
    (48000, 24000): (1, 2, 256, 64, 64, 0, 50692),
    (16000, 24000): (3, 2, 128, 64, 32, 0, 42244),
    (22050, 24000): (160, 147, 128, 64, 1, 0, 80388),
    (8000, 24000): (3, 1, 128, 64, 32, 0, 34052),
    (24000, 16000): (2, 3, 192, 64, 32, 0, 42244),
    (44100, 16000): (160, 441, 360, 16, 1, 0, 40228),
    (11025, 32000): (1280, 441, 128, 4, 1, 0, 28692),
    (32000, 11025): (441, 1280, 376, 4, 2, 28, 57020),
    (96000, 11025): (147, 1280, 1120, 4, 2, 52, 50292),
    (96000, 44100): (147, 320, 280, 16, 2, 16, 61488),
    (16000, 11025): (441, 640, 192, 16, 1, 48, 70836),
    (96000, 8000): (1, 12, 1536, 64, 16, 0, 59524),
}


def lds_bytes(L, M, taps, rounds):
    """twv_resample.hip's carve restated: rounds * M + taps staged inputs, L * rounds gathered outputs spread by o + o / 32, one pad"""
    o = L * rounds
    return 4 * (rounds * M + taps + o + o // 32 + 1)


def ratio(sr_in, sr_out):
    g = gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def out_samples(n_in, sr_in, sr_out):
    L, M = ratio(sr_in, sr_out)
    return -((-int(n_in) * L) // M)


def h(u):
    u = np.asarray(u, np.float64)
    inside = np.abs(u) < ZEROS
    z = np.where(inside, u / ZEROS, 0.0)
    return np.where(inside, ROLLOFF * np.sinc(ROLLOFF * u) * np.i0(BETA * np.sqrt(1.0 - z * z)) / np.i0(BETA), 0.0)


def half_width(sr_in, sr_out):
    """input samples on either side of the position that can carry weight: ceil(Z / s)"""
    L, M = ratio(sr_in, sr_out)
    return ZEROS if L >= M else -((-ZEROS * M) // L)


def coefficients(sr_in, sr_out, W=None):
    """(L, 2W) float64: c[p][k] = s h(s (k - W + p / L)), the weight of x[q + W - k] in an output of phase p; columns a wider W adds
    are 0 by h's support"""
    L, M = ratio(sr_in, sr_out)
    s = min(1.0, L / M)
    W = half_width(sr_in, sr_out) if W is None else int(W)
    assert W >= half_width(sr_in, sr_out)
    k = np.arange(2 * W)[None, :]
    p = np.arange(L)[:, None]
    return s * h(s * (((k - W) * L + p) / L))


def resample(x, sr_in, sr_out, dtype=np.float64):
    """-> float64 array of out_samples(len(x)) values (computed in `dtype`)"""
    L, M = ratio(sr_in, sr_out)
    W = half_width(sr_in, sr_out)
    c = coefficients(sr_in, sr_out).astype(dtype)
    x = np.asarray(x, np.float64).astype(dtype)
    n_out = out_samples(len(x), sr_in, sr_out)
    xp = np.concatenate([np.zeros(2 * W, dtype), x, np.zeros(2 * W + M, dtype)])
    y = np.zeros(n_out, np.float64)
    back = W - np.arange(2 * W)                       # x[q + W - k]
    for p0 in range(min(L, n_out)):                   # outputs t = p0, p0 + L, ...: one coefficient row
        t = np.arange(p0, n_out, L, dtype=np.int64)
        q = (t * M) // L
        row = c[(p0 * M) % L]
        prod = xp[(q[:, None] + back[None, :]) + 2 * W] * row[None, :]
        y[t] = prod.sum(axis=1, dtype=dtype)
    return y


def bar(x, sr_in, sr_out):
    """-> (float64 result, the bar for max|device - float64|, the float32 checker's own distance)"""
    y64 = resample(x, sr_in, sr_out)
    d32 = np.abs(resample(x, sr_in, sr_out, dtype=np.float32) - y64).max() if len(y64) else 0.0
    peak = np.abs(y64).max() if len(y64) else 0.0
    return y64, max(RATIO * d32, FLOOR * peak), d32


def poly_taps(sr_in, sr_out):
    """the same definition as one prototype filter for scipy.signal.resample_poly(x, L, M, window=taps) (scipy multiplies a given
    window by `up`, hence the / L): taps[k] = s h(s k / L) / L, k = -K .. K, K = ceil(Z L / s)"""
    L, M = ratio(sr_in, sr_out)
    s = min(1.0, L / M)
    K = int(np.ceil(ZEROS * L / s))
    k = np.arange(-K, K + 1)
    return s * h(s * k / L) / L
