"""No GPU: the yardstick of the Griffin-Lim tests (the float32 run of the checker), proof that their bar sees a truncated
de-emphasis, and twv_griffin_lim_create's argument checks (host-only: create touches no device)."""
import ctypes as C

import numpy as np
import pytest

import audio_analysis_ref as R
import griffin_lim_cases as G
from oracle import audio_np as A


def _every_case():
    for geo in G.GEOMETRIES:
        for iters in (0, 3):
            yield "geometry %s iters %d" % (geo, iters), G.geometry_case(geo, iters)[3]
    n_fft, win, hop, T = G.LONG
    spec, u = G.inputs(n_fft, T, 2, G.seed_of(G.LONG, G.LONG_ITERS))
    for k in G.DEEMPH_KS:
        hp = G.hparams(n_fft, win, hop, G.LONG_ITERS, k)
        yield "long k %g" % k, [G.checkers(spec[b], u[b], hp, G.LONG_ITERS, key=(G.LONG, G.LONG_ITERS, 2, k, b)) for b in range(2)]
    for geo in G.EDGES:
        yield "chunk edge %s" % (geo,), G.geometry_case(geo, 2, B=1, k=G.EDGE_K)[3]


def test_float32_checker_stays_near_the_float64_checker():
    """the yardstick itself: every stage in float32 / complex64, within 1e-5 of the peak of the float64 checker at every case of the
    geometry table, every k of the de-emphasis cases and both chunk-edge lengths -- inputs the restatement itself handles"""
    worst = 0.0
    for name, pairs in _every_case():
        for b, (y64, y32) in enumerate(pairs):
            assert y32.dtype == np.float32 and y64.dtype == np.float64 and y32.shape == y64.shape
            e = G.rel(y32, y64)
            print("%-40s utterance %d: e_f32 = %.3e" % (name, b, e))
            worst = max(worst, e)
            assert e <= 1e-5, (name, b, e)
    assert worst > 1e-8, "a float32 run cannot sit on the float64 one: the float32 path is not float32"


def test_float32_recurrence_is_the_float64_one_rounded():
    x = np.random.RandomState(3).randn(500).astype(np.float32)
    y32, y64 = R.inv_preemphasis_f32(x, 0.97), A.inv_preemphasis(x.astype(np.float64), 0.97)
    assert y32.dtype == np.float32 and 0 < np.abs(y32 - y64).max() <= 1e-5 * np.abs(y64).max()
    from scipy.signal import lfilter
    assert np.abs(lfilter([1.0], [1.0, -0.97], x.astype(np.float64)) - y64).max() <= 1e-12 * np.abs(y64).max()


@pytest.mark.parametrize("k,seen", [(0.97, False), (0.995, True), (0.999, True)])
def test_bar_sees_a_truncated_deemphasis(k, seen):
    """A numpy model of the de-emphasis as it was (2048-sample chunks, each restarted from a zero state 1024 samples earlier) on the
    float64 checker's pre-de-emphasis signal of the long case (5950 samples, three chunks): at k = 0.995 and 0.999 it lies outside
    the bar that the GPU tests hold the device to, at k = 0.97 (k^1024 = 3e-14) inside.  The bar is taken from the float32
    checker's distance on the same utterance, as the GPU tests take it."""
    n_fft, win, hop, T = G.LONG
    x = G.long_pre_deemphasis(0)
    assert len(x) == 5950
    spec, u = G.inputs(n_fft, T, 2, G.seed_of(G.LONG, G.LONG_ITERS))
    hp = G.hparams(n_fft, win, hop, G.LONG_ITERS, k)
    y64, y32 = G.checkers(spec[0], u[0], hp, G.LONG_ITERS, key=(G.LONG, G.LONG_ITERS, 2, k, 0))
    assert np.abs(A.inv_preemphasis(x, k) - y64).max() == 0.0
    e_model, bar = G.rel(R.chunked_deemphasis_model(x, k), y64), G.bar(G.rel(y32, y64))
    print("k = %g: truncated de-emphasis %.3e of the peak, bar %.3e (k^1024 = %.1e)" % (k, e_model, bar, k ** 1024))
    assert bar <= G.OLD_BAR
    assert (e_model > bar) == seen, (k, e_model, bar)
    # exact where nothing is truncated: one chunk, or a warm-up that reaches the start of the row
    assert np.array_equal(R.chunked_deemphasis_model(x[:2048], k), A.inv_preemphasis(x[:2048], k))
    assert np.array_equal(R.chunked_deemphasis_model(x, k, warm=len(x)), A.inv_preemphasis(x, k))


def _create(*args):
    from twvk_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.twv_griffin_lim_create(*args, C.byref(h))
    if rc == 0:
        n = L.twv_griffin_lim_samples(h)
        L.twv_griffin_lim_destroy(h)
        return rc, n
    return rc, None


def test_create_argument_checks():
    """n_fft 64: hop * (T - 1) = 32 = n_fft/2 is refused (the reflection would read past the signal), 33 is the shortest accepted"""
    TWV_E_INVALID = 1
    assert _create(64, 11, 64, 4, 1) == (0, 33)
    assert _create(64, 33, 64, 2, 1) == (0, 33)
    assert _create(64, 8, 64, 5, 1)[0] == TWV_E_INVALID              # 8 * 4 = 32
    assert _create(64, 32, 64, 2, 1)[0] == TWV_E_INVALID
    assert _create(64, 16, 65, 20, 1)[0] == TWV_E_INVALID            # win > n_fft
    assert _create(63, 16, 32, 20, 1)[0] == TWV_E_INVALID            # odd n_fft
    assert _create(64, 64, 64, 1, 1)[0] == TWV_E_INVALID             # T = 1
    assert _create(64, 16, 64, 20, 0)[0] == TWV_E_INVALID
    assert _create(64, 16, 64, 20, 3) == (0, 16 * 19)


@pytest.mark.parametrize("k", [1.0001, -1.5, float("nan"), float("inf")])
def test_preemphasis_outside_the_contract_is_refused_before_any_launch(k):
    """include/twv_amd.h: the de-emphasis is computed for k in [-1, 1]; anything else is TWV_E_INVALID, the first thing both fronts
    check (no buffer is passed here, so nothing could be launched; the message tells this refusal from the one for the buffers)"""
    from twvk_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_griffin_lim_create(64, 16, 64, 20, 1, C.byref(h)))
    try:
        assert L.twv_inv_linear_spectrogram(h, None, None, 0, 1.5, 20.0, 4.0, -100.0, k, None, None, None) == 1
        assert b"preemphasis" in L.twv_last_error()
        assert L.twv_inv_linear_spectrogram(h, None, None, 0, 1.5, 20.0, 4.0, -100.0, 1.0, None, None, None) == 1
        assert b"preemphasis" not in L.twv_last_error()              # k = 1 is inside the contract: refused for the buffers alone
        assert L.twv_inv_spectrogram(h, None, 33, None, None, 0, 1.5, 20.0, 4.0, -100.0, 1, k, None, None, None) == 1
        assert b"preemphasis" in L.twv_last_error()
    finally:
        L.twv_griffin_lim_destroy(h)
