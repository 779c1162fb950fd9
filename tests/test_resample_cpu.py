"""No device: the resampling contract's checker (tests/resample_ref.py) against scipy.signal.resample_poly -- a second, independently
written implementation of the same definition -- and the host side of the C-ABI (twv_resample_create and what it computes)."""
import ctypes as C

import numpy as np
import pytest

import resample_ref as R


def _create(sr_in, sr_out, max_in=1000, batch=1):
    from twvk_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.twv_resample_create(sr_in, sr_out, max_in, batch, C.byref(h))
    return L, h, rc


@pytest.mark.parametrize("pair", R.PAIRS, ids=lambda p: "%d-%d" % p)
def test_checker_equals_resample_poly(pair):
    """bar: 1e-12 of the peak (two float64 sums of the same products in different orders)"""
    from scipy.signal import resample_poly
    sr_in, sr_out = pair
    L, M = R.ratio(sr_in, sr_out)
    taps = R.poly_taps(sr_in, sr_out)
    rng = np.random.RandomState(sr_in % 997 + sr_out)
    for n in (1, 2, 147, 148, 2003):
        x = rng.uniform(-1, 1, n)
        want = resample_poly(x, L, M, window=taps)
        got = R.resample(x, sr_in, sr_out)
        assert len(got) == len(want) == R.out_samples(n, sr_in, sr_out) == int(np.ceil(n * L / M))
        d, peak = np.abs(got - want).max(), np.abs(want).max()
        assert d <= 1e-12 * peak, (pair, n, d, peak)


def test_create_is_host_only_for_every_standard_pair():
    """all 72 ordered pairs of the nine standard rates: phases = L, taps = 2 * (ceil(Z / s) rounded up to a multiple of 4), the table
    against the checker's float64 coefficients to one float32 spacing of the largest coefficient (another I0 evaluation, no more)"""
    n = 0
    for sr_in in R.RATES:
        for sr_out in R.RATES:
            if sr_in == sr_out:
                continue
            L, h, rc = _create(sr_in, sr_out)
            assert rc == 0, (sr_in, sr_out, L.twv_last_error())
            try:
                up, down = R.ratio(sr_in, sr_out)
                assert L.twv_resample_phases(h) == up
                W = (R.half_width(sr_in, sr_out) + 3) // 4 * 4
                taps = L.twv_resample_taps(h)
                assert taps == 2 * W
                for n_in in (0, 1, down, down + 1, 2 * down - 1, 12345):
                    assert L.twv_resample_out_samples(h, n_in) == -((-n_in * up) // down) == R.out_samples(n_in, sr_in, sr_out)
                assert L.twv_resample_workspace_bytes(h) >= up * taps * 4
                assert L.twv_resample_kernel_name(h).decode().startswith("rs_resample_kernel<")
                tab = np.empty((up, taps), np.float32)
                assert L.twv_resample_filter_host(h, tab.ctypes.data_as(C.c_void_p)) == 0
                want = R.coefficients(sr_in, sr_out, W)
                assert np.abs(tab - want).max() <= np.spacing(np.float32(np.abs(want).max())), (sr_in, sr_out)
                edge = W - R.half_width(sr_in, sr_out)               # the columns the rounding of W adds
                assert not tab[:, :edge].any() and not tab[:, taps - edge:].any()
            finally:
                L.twv_resample_destroy(h)
            n += 1
    assert n == 72


def test_every_route_of_the_kernel_has_its_pair():
    """resample_ref.ROUTES is what twv_resample_create decides for the pairs the GPU tests iterate (LR from the kernel's name, rounds =
    LR * chunks from twv_resample_rounds, L and taps from their accessors), and over the table every instantiation, chunks > 1 at the
    two narrow ones, lanes that are not live at both, a tile above 64 KiB at <16> and the long rows keep a pair: a retuning of the
    carve that moves a pair to another route fails here instead of silently dropping the GPU suite's cover of the route it left."""
    assert set(R.ROUTES) == set(R.PAIRS) and len(R.PAIRS) == 13
    seen = {}
    for pair in R.PAIRS:
        up, down, taps, lr, chunks, dead, lds = R.ROUTES[pair]
        assert (up, down) == R.ratio(*pair)
        L, h, rc = _create(*pair)
        assert rc == 0, (pair, L.twv_last_error())
        try:
            assert L.twv_resample_phases(h) == up and L.twv_resample_taps(h) == taps, pair
            assert L.twv_resample_kernel_name(h).decode() == "rs_resample_kernel<%d>" % lr, pair
            assert L.twv_resample_rounds(h) == lr * chunks, pair
        finally:
            L.twv_resample_destroy(h)
        lanes = 64 // lr                                          # phases a wave has in flight
        assert dead == (lanes - up % lanes) % lanes * lr, pair
        assert lds == R.lds_bytes(up, down, taps, lr * chunks) <= 80 * 1024, pair
        seen.setdefault(lr, []).append((chunks, up % lanes != 0, lds, taps, up >= down))
    assert set(seen) == {64, 16, 4}
    for lr in (16, 4):
        assert any(c > 1 for c, _, _, _, _ in seen[lr]), "chunks > 1 at LR %d" % lr
        assert any(d for _, d, _, _, _ in seen[lr]), "lanes that are not live at LR %d" % lr
    assert any(c > 1 for c, _, _, _, _ in seen[64])
    assert any(lds > 64 * 1024 for _, _, lds, _, _ in seen[16]), "a tile above 64 KiB at LR 16"
    assert any(t == 1120 for _, _, _, t, _ in seen[4]) and any(t == 1536 for _, _, _, t, _ in seen[64]), "the long rows"
    assert any(u for _, _, _, _, u in seen[4]), "upsampling at LR 4"


def test_kernel_is_in_the_library():
    import subprocess
    from twvk_amd import _lib
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "rs_resample_kernel" in nm, "the gfx950 resampling kernel must be in the library"


@pytest.mark.parametrize("args", [(24000, 24000, 100, 1), (0, 24000, 100, 1), (44100, -1, 100, 1), (44100, 24000, 0, 1), (44100, 24000, 100, 0)],
                         ids=["equal", "zero-rate", "negative-rate", "no-samples", "no-batch"])
def test_create_refuses(args):
    L, h, rc = _create(*args)
    assert rc == 1 and h.value is None, (rc, L.twv_last_error())                        # TWV_E_INVALID


def test_create_refuses_a_ratio_beyond_the_table_cap():
    L, h, rc = _create(44101, 24000)                  # coprime: 24000 phases x 240 taps
    assert rc == 2 and h.value is None and b"table" in L.twv_last_error()               # TWV_E_UNSUPPORTED


def test_lengths_above_max_samples_in_are_refused_before_any_device_work():
    """twv_resample validates on the host first: the pointers are never touched"""
    L, h, rc = _create(44100, 24000, max_in=1000, batch=2)
    assert rc == 0
    try:
        lengths = np.asarray([1000, 1001], np.int32)
        rc = L.twv_resample(h, C.c_void_p(256), 0, 1, lengths.ctypes.data_as(C.c_void_p), C.c_void_p(256), C.c_void_p(256), None)
        assert rc == 1 and b"longer than max_samples_in" in L.twv_last_error()
        for fmt, ch in ((2, 1), (0, 3), (-1, 1), (0, 0)):
            assert L.twv_resample(h, C.c_void_p(256), fmt, ch, None, C.c_void_p(256), C.c_void_p(256), None) == 1
    finally:
        L.twv_resample_destroy(h)


def test_equal_rates_return_the_input_and_read_wav_still_refuses(tmp_path):
    from scipy.io import wavfile
    from twvk_amd import audio, preprocess
    x = np.arange(5, dtype=np.float32)
    got, lengths = audio.resample(x, 24000, 24000)
    assert got is x and lengths is None
    wavfile.write(str(tmp_path / "u9.wav"), 16000, np.zeros(4000, np.int16))
    with pytest.raises(ValueError, match="resampling is not built"):
        preprocess.read_wav(str(tmp_path / "u9.wav"), 24000)
    # at the file's own rate load_wav needs no device and reads what read_wav reads
    wavfile.write(str(tmp_path / "u8.wav"), 24000, (np.arange(-300, 300).reshape(-1, 2) * 50).astype(np.int16))
    assert np.array_equal(audio.load_wav(str(tmp_path / "u8.wav"), 24000), preprocess.read_wav(str(tmp_path / "u8.wav"), 24000))
