"""No GPU: the ragged Griffin-Lim interface (twv_griffin_lim_create_ragged and its accessors are host-only), the argument checks of
the list fronts in audio.py, the cap on the bar of every case of tests/griffin_lim_ragged_cases.py, and proof that padding to the
longest utterance is no substitute for per-utterance boundaries."""
import ctypes as C
import os

import numpy as np
import pytest

import griffin_lim_cases as G
import griffin_lim_ragged_cases as RG

TWV_E_INVALID = 1
NAMES = ["twv_griffin_lim_create_ragged", "twv_griffin_lim_total_frames", "twv_griffin_lim_total_samples", "twv_griffin_lim_offsets"]


def _lib():
    from twvk_amd import _lib
    return _lib, _lib.lib()


def _create_ragged(n_fft, hop, win, frames, batch=None):
    """-> (rc, handle or None, last error)"""
    _, L = _lib()
    h = C.c_void_p()
    arr = None if frames is None else np.asarray(frames, np.int32)
    rc = L.twv_griffin_lim_create_ragged(n_fft, hop, win, None if arr is None else arr.ctypes.data_as(C.c_void_p),
                                         len(arr) if batch is None else batch, C.byref(h))
    return rc, (h if rc == 0 else None), L.twv_last_error()


def _offsets(L, h, batch):
    f, s = (C.c_int64 * (batch + 1))(), (C.c_int64 * (batch + 1))()
    assert L.twv_griffin_lim_offsets(h, C.cast(f, C.c_void_p), C.cast(s, C.c_void_p)) == 0
    return list(f), list(s)


def test_the_four_names_are_in_the_header_and_exported():
    lib, L = _lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    for name in NAMES:
        assert name + "(" in header and name in lib.EXPORTS and hasattr(L, name), name


def test_create_ragged_refusals():
    """create's rules for every utterance; the message names the utterance at fault"""
    rc, h, _ = _create_ragged(64, 16, 64, None, batch=3)
    assert rc == TWV_E_INVALID and h is None                                     # NULL list
    assert _create_ragged(64, 16, 64, [20, 20], batch=0)[0] == TWV_E_INVALID
    rc, _, err = _create_ragged(64, 64, 64, [20, 9, 1, 20])                      # a length of 1
    assert rc == TWV_E_INVALID and b"utterance 2" in err
    rc, _, err = _create_ragged(64, 8, 64, [20, 5])                              # 8 * 4 = 32 = n_fft/2: at the reflect padding
    assert rc == TWV_E_INVALID and b"utterance 1" in err and b"reflect" in err
    rc, _, err = _create_ragged(64, 8, 64, [4, 20])                              # 24: under it
    assert rc == TWV_E_INVALID and b"utterance 0" in err and b"reflect" in err
    assert _create_ragged(64, 16, 65, [20, 20])[0] == TWV_E_INVALID              # win > n_fft
    assert _create_ragged(63, 16, 32, [20, 20])[0] == TWV_E_INVALID              # odd n_fft
    # the shortest accepted stays accepted inside a batch: 11 * 3 = 33 = n_fft/2 + 1
    _, L = _lib()
    rc, h, _ = _create_ragged(64, 11, 64, [4, 9, 4])
    assert rc == 0
    L.twv_griffin_lim_destroy(h)
    # more frames than one hipFFT plan takes: 2 x (2^30 + 1) frames (host arithmetic only: nothing is allocated)
    rc, _, err = _create_ragged(64, 1, 64, [2 ** 30 + 1, 2 ** 30 + 1])
    assert rc == TWV_E_INVALID and b"hipFFT" in err


def test_offsets_and_totals():
    _, L = _lib()
    rc, h, _ = _create_ragged(128, 25, 101, [21, 4, 9])
    assert rc == 0
    try:
        assert _offsets(L, h, 3) == ([0, 21, 25, 34], [0, 500, 575, 775])
        assert L.twv_griffin_lim_total_frames(h) == 34 and L.twv_griffin_lim_total_samples(h) == 775
        assert L.twv_griffin_lim_samples(h) == 500                               # the longest utterance's
        f, s = _offsets(L, h, 3)
        assert all(s[b] == 25 * (f[b] - b) for b in range(4))
        assert L.twv_griffin_lim_offsets(h, None, None) == 0                     # either pointer may be NULL
    finally:
        L.twv_griffin_lim_destroy(h)


def test_uniform_handle_answers_the_new_accessors_and_its_workspace_is_unchanged():
    lib, L = _lib()
    h = C.c_void_p()
    lib.check(L.twv_griffin_lim_create(128, 25, 101, 21, 3, C.byref(h)))
    rc, r, _ = _create_ragged(128, 25, 101, [21, 21, 21])
    assert rc == 0
    try:
        assert _offsets(L, h, 3) == ([0, 21, 42, 63], [0, 500, 1000, 1500]) == _offsets(L, r, 3)
        assert L.twv_griffin_lim_total_frames(h) == 63 and L.twv_griffin_lim_total_samples(h) == 1500
        assert L.twv_griffin_lim_samples(h) == L.twv_griffin_lim_samples(r) == 500
        bf, nbin, n_fft, nchunk = 63, 65, 128, 1
        uniform = bf * nbin * 4 + bf * nbin * 8 * 2 + bf * n_fft * 4 + 3 * 500 * 4 + 3 * nchunk * 4 + 4096
        assert L.twv_griffin_lim_workspace_bytes(h) == uniform                   # the formula it had before the ragged handles
        table = L.twv_griffin_lim_workspace_bytes(r) - uniform
        assert 3 * 4 * 8 <= table <= 3 * 4 * 8 + 256                             # three arrays of batch + 1 64-bit offsets
    finally:
        L.twv_griffin_lim_destroy(h)
        L.twv_griffin_lim_destroy(r)


@pytest.mark.parametrize("k", [1.5, float("nan")])
def test_preemphasis_outside_the_contract_is_refused_on_a_ragged_handle(k):
    _, L = _lib()
    rc, h, _ = _create_ragged(64, 16, 64, [20, 4, 9])
    assert rc == 0
    try:
        assert L.twv_inv_linear_spectrogram(h, None, None, 0, 1.5, 20.0, 4.0, -100.0, k, None, None, None) == TWV_E_INVALID
        assert b"preemphasis" in L.twv_last_error()
        assert L.twv_inv_linear_spectrogram(h, None, None, 0, 1.5, 20.0, 4.0, -100.0, 1.0, None, None, None) == TWV_E_INVALID
        assert b"preemphasis" not in L.twv_last_error()                          # k = 1 is inside: refused for the buffers alone
        assert L.twv_inv_spectrogram(h, None, 33, None, None, 0, 1.5, 20.0, 4.0, -100.0, 1, k, None, None, None) == TWV_E_INVALID
        assert b"preemphasis" in L.twv_last_error()
    finally:
        L.twv_griffin_lim_destroy(h)


def test_list_fronts_raise_value_errors_without_a_device():
    from twvk_amd.audio import inv_linear_spectrogram_list, inv_mel_spectrogram_list
    hp = G.hparams(64, 64, 16, 0)
    F = 33
    ok = [np.zeros((9, F), np.float32), np.zeros((4, F), np.float32)]
    with pytest.raises(ValueError):
        inv_linear_spectrogram_list([], hp)
    with pytest.raises(ValueError, match="utterance 1"):
        inv_linear_spectrogram_list([ok[0], np.zeros((4, F + 1), np.float32)], hp)           # a wrong channel count
    with pytest.raises(ValueError):
        inv_linear_spectrogram_list([np.zeros((2, 9, F), np.float32)], hp)                   # a batch is not an utterance
    with pytest.raises(ValueError, match="uniforms"):
        inv_linear_spectrogram_list(ok, hp, uniforms=[np.zeros((9, F), np.float32), np.zeros((5, F), np.float32)])
    with pytest.raises(ValueError, match="uniforms"):
        inv_linear_spectrogram_list(ok, hp, uniforms=[np.zeros((9, F), np.float32)])
    with pytest.raises(ValueError, match="utterance 1"):
        inv_linear_spectrogram_list([ok[0], np.zeros((3, F), np.float32)], hp)               # 16 * 2 = 32 = fft_size/2
    with pytest.raises(ValueError, match="utterance 0"):
        inv_linear_spectrogram_list([np.zeros((1, F), np.float32), ok[1]], hp)
    with pytest.raises(ValueError, match="use_lws"):
        inv_linear_spectrogram_list(ok, G.hparams(64, 64, 16, 0, use_lws=True))
    num_mels, basis, _ = RG.mel_setup()
    hpm = G.hparams(64, 64, 16, 0, num_mels=num_mels)
    mels = [np.zeros((9, num_mels), np.float32), np.zeros((4, num_mels), np.float32)]
    with pytest.raises(ValueError):
        inv_mel_spectrogram_list([], hpm, mel_basis=basis)
    with pytest.raises(ValueError, match="utterance 1"):
        inv_mel_spectrogram_list([mels[0], ok[1]], hpm, mel_basis=basis)                     # linear channels given to the mel front
    with pytest.raises(ValueError, match="basis"):
        inv_mel_spectrogram_list(mels, hpm, mel_basis=basis[:, :20])
    with pytest.raises(ValueError, match="use_lws"):
        inv_mel_spectrogram_list(mels, G.hparams(64, 64, 16, 0, num_mels=num_mels, use_lws=True), mel_basis=basis)
    with pytest.raises(ValueError, match="utterance 1"):
        inv_mel_spectrogram_list([mels[0], np.zeros((3, num_mels), np.float32)], hpm, mel_basis=basis)


def test_synthesize_refuses_an_unknown_griffin_lim_value_before_anything_runs():
    from twvk_amd.synthesizer import Synthesizer
    with pytest.raises(ValueError, match="griffin_lim"):
        Synthesizer().synthesize(tokens=[[5, 1]], griffin_lim="padded")


@pytest.mark.parametrize("name", sorted(RG.CASES))
def test_bar_of_every_case_is_capped(name):
    """the cap on the bar, without a GPU: no utterance of any row may be given more than G.OLD_BAR; the checker pair agrees on the
    utterance's length, hop * (T_i - 1)"""
    (n_fft, win, hop), Ts, _, _, _ = RG.CASES[name]
    for iters, k in RG.rows_of(name):
        hp, specs, us, pairs, _ = RG.case(name, iters, k)
        assert len(specs) == len(us) == len(pairs) == len(Ts)
        for i, (y64, y32) in enumerate(pairs):
            assert y64.shape == y32.shape == (hop * (Ts[i] - 1),) and specs[i].shape[0] == us[i].shape[0] == Ts[i]
            e_f32 = G.rel(y32, y64)
            assert 0 < G.bar(e_f32) <= G.OLD_BAR, (name, iters, k, i, e_f32)
    if name == "I":
        assert sum(Ts) * (n_fft // 2 + 1) > 65535 * 256 and sum(Ts) * n_fft > 65535 * 256    # past ga_grid's clamp
    if name == "G":
        assert [hop * (t - 1) for t in Ts] == [2048, 2080, 4128, 288]


@pytest.mark.parametrize("geometry,T,T_pad,iters", RG.PADDED, ids=lambda v: str(v).replace(" ", ""))
def test_padding_to_the_longest_is_far_outside_the_bar(geometry, T, T_pad, iters):
    """pad the trimmed frames with -max_abs_value, run, cut back: more than G.OLD_BAR (and so than any bar) away from the utterance's
    own run -- an indexing slip across an utterance boundary cannot hide inside a bar"""
    e, bar = RG.padded_then_cut(geometry, T, T_pad, iters)
    print("%s frames %d -> %d iters %d: %.3f of the peak, bar %.1e" % (geometry, T, T_pad, iters, e, bar))
    assert bar <= G.OLD_BAR < e
